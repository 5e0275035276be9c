"""Incremental batches on the device bit packer (lamehip_batch_set_incremental_packing, csrc/lh_drain.hip) on the GPU: after
every round every stream drains what the host-packed incremental batch fed the same calls drains -- and what the entry point
returned, call by call --; rounds in windows and on changing kernels against the one-shot device-packed batch; a backlog of
undrained rounds, too small buffers and the bytes in place; conversion and ReplayGain round by round on top, fed from a
tensor; the lifecycle and what stays refused."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import lamehip
import pcm_input_support as psup
import test_pcm_input_device as t
from lamehip import PCM_F32, PCM_F32_UNIT, PCM_S16, PCM_S32
from test_append_input_device import CHUNKS, EntryPoint, append_chunk
from test_incremental_packing import landing_frames, parse_frames

pytestmark = pytest.mark.gpu

# (id, sample type, rate, settings): the streams go through the entry point the sample type is named after
CASES = [
    ("cbr128-js", PCM_F32_UNIT, 44100, dict(brate=128, mode=1)),
    ("vbr3", PCM_F32, 44100, dict(vbr_q=3)),
    ("mono96", PCM_S32, 44100, dict(brate=96, channels=1)),
    ("cbr320-48k", PCM_F32_UNIT, 48000, dict(brate=320)),
    ("mpeg2-22k-cbr64", PCM_F32_UNIT, 22050, dict(brate=64)),
    ("mpeg25-8k-cbr16", PCM_F32_UNIT, 8000, dict(brate=16)),
]


def packed_batch(enc, stype, B, cap):
    b = lamehip.Batch(enc, B, cap)
    if stype != PCM_S16:
        b.set_sample_type(stype)
    b.set_device_packing()
    b.set_incremental_packing()
    return b


def host_batch(enc, stype, B, cap):
    b = lamehip.Batch(enc, B, cap)
    if stype != PCM_S16:
        b.set_sample_type(stype)
    return b


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_rounds_match_the_host_packer_and_the_entry_point(case):
    """eight streams of 0.9 s + 37 s samples in ragged chunks (also empty ones): after every encode_available and after
    finish every stream's drain is the host-packed incremental batch's, and the entry point's return value for the call"""
    _, stype, sr, kw = CASES[case]
    B = 8
    rng = np.random.default_rng(8800 + case)
    lens = [int(sr * 0.9) + 37 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9900 + 10 * case + s, lens[s], sr) for s in range(B)]
    eps = [EntryPoint(stype, False, sr, kw) for _ in range(B)]
    enc = t.open_product(sr, kw)
    dev, host = packed_batch(enc, stype, B, max(lens) + case % 4), host_batch(enc, stype, B, max(lens) + case % 4)
    pos, rounds, total, ms = [0] * B, 0, 0, 0.0
    while any(pos[s] < lens[s] for s in range(B)):
        want = []
        for s in range(B):
            n = min(int(rng.choice(CHUNKS)), lens[s] - pos[s])
            x = xs[s][:, pos[s]:pos[s] + n]
            want.append(eps[s].call(x))
            for b in (dev, host):
                append_chunk(b, s, x, False, enc.channels == 1)
            pos[s] += n
        assert dev.encode_available() == host.encode_available()
        ms += dev.drain_ms()
        for s in range(B):
            got = dev.drain(s)
            assert got == host.drain(s), "round %d stream %d (host packer)" % (rounds, s)
            assert got == want[s], "round %d stream %d (entry point)" % (rounds, s)
            total += len(got)
        rounds += 1
    assert dev.finish() == host.finish()
    for s in range(B):
        got = dev.drain(s)
        assert got == host.drain(s), "flush of stream %d (host packer)" % s
        assert got == eps[s].flush(), "flush of stream %d (entry point)" % s
        assert dev.frames(s) == host.frames(s)
    assert rounds >= 2 and total > 8 * 1000 and ms > 0.0
    dev.close()
    host.close()
    enc.close()


def s16_rounds(enc, make, xs, plan, landing_check=None):
    """the drains of batch make() fed xs by `plan' (rounds of per-stream counts), round by round, then the flush's"""
    B = len(xs)
    b = make()
    pos, out = [0] * B, []
    for ns in plan:
        for s in range(B):
            if ns[s] is not None:
                b.append(s, xs[s][0, pos[s]:pos[s] + ns[s]], xs[s][1, pos[s]:pos[s] + ns[s]])
                pos[s] += ns[s]
        b.encode_available()
        out.append([b.drain(s) for s in range(B)])
    assert pos == [x.shape[1] for x in xs]
    b.finish()
    out.append([b.drain(s) for s in range(B)])
    b.close()
    return out


def ragged_plan(rng, lens, first=None):
    """rounds of chunks from CHUNKS until every stream is through; first: stream 0's fixed chunk for its first eight rounds"""
    pos, plan = [0] * len(lens), []
    while any(p < n for p, n in zip(pos, lens)):
        ns = [min(int(rng.choice(CHUNKS)), lens[s] - pos[s]) for s in range(len(lens))]
        if first is not None and len(plan) < 8:
            ns[0] = min(first, lens[0] - pos[0])
        pos = [p + n for p, n in zip(pos, ns)]
        plan.append(ns)
    return plan


def no_reservoir(sr):
    enc = lamehip.Encoder.__new__(lamehip.Encoder)
    lib = enc.lib = lamehip.load_library()
    enc.h = C.c_void_p(lib.lame_init())
    enc.channels = 2
    lib.lame_set_in_samplerate(enc.h, sr)
    lib.lame_set_bWriteVbrTag(enc.h, 0)
    lib.lame_set_brate(enc.h, 128)
    lib.lame_set_disable_reservoir(enc.h, 1)
    assert lib.lame_init_params(enc.h) == 0, lamehip.last_error()
    assert enc.config().disable_reservoir == 1
    return enc


@pytest.mark.parametrize("what", ["abr112-silence", "no-reservoir"])
def test_rounds_match_the_host_packer_on_settings_of_the_handle(what):
    """ABR 112 with one stream of digital silence fed a frame's worth per round for its first eight rounds -- a frame
    without main data ends on a queued header, and the round hands out nothing of it, as the reference does --, and CBR
    with the reservoir disabled: every round's drains are the host-packed batch's"""
    sr, B = 44100, 8
    rng = np.random.default_rng(8900)
    lens = [int(sr * 0.9) + 37 * s for s in range(B)]
    xs = [helpers.synth_stream(9950 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    if what == "abr112-silence":
        enc = lamehip.Encoder(sr, abr=112)
        xs[0] = np.zeros_like(xs[0])
        plan = ragged_plan(rng, lens, first=1152)
    else:
        enc = no_reservoir(sr)
        plan = ragged_plan(rng, lens)
    cap = max(lens)

    def device():
        b = lamehip.Batch(enc, B, cap)
        b.set_device_packing()
        b.set_incremental_packing()
        return b

    got = s16_rounds(enc, device, xs, plan)
    want = s16_rounds(enc, lambda: lamehip.Batch(enc, B, cap), xs, plan)
    for r, (g, w) in enumerate(zip(got, want)):
        for s in range(B):
            assert g[s] == w[s], "round %d stream %d" % (r, s)
    assert sum(len(x) for r in want for x in r) > 8 * 5000
    if what == "abr112-silence":
        # the silent stream's frames whose main data ends on a queued header, from the expected bytes' own headers; after
        # round k (k >= 1, counted from 0) of 1152 samples each the stream's last encoded frame is k - 1
        cfg = enc.config()
        landing = landing_frames(parse_frames(b"".join(r[0] for r in want), cfg), cfg.sideinfo_len)
        ended_on = [k - 1 for k in range(1, 8) if k - 1 in landing]
        assert ended_on, sorted(landing)
        for k in ended_on:
            assert want[k][0] == b""
    enc.close()


def test_windows_and_changing_kernels_give_the_one_shot_bytes(monkeypatch):
    """LAMEHIP_MID_WINDOW and LAMEHIP_SPLIT_DENY alternate between the rounds: launches in windows of frames, on the split
    pipeline and on the fused kernel work on one packer state -- the bytes of the one-shot device-packed batch"""
    sr, B = 44100, 4
    enc = t.open_product(sr, dict(brate=128))
    lens = [int(0.8 * sr) + 4111 * s for s in range(B)]
    xs = [helpers.synth_stream(9960 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    one = lamehip.Batch(enc, B, max(lens) + 3)
    one.set_device_packing()
    for s, x in enumerate(xs):
        one.set_pcm(s, x[0], x[1])
    one.encode()
    want = [one.get_bytes(s) for s in range(B)]
    one.close()
    b = lamehip.Batch(enc, B, max(lens) + 3)
    b.set_device_packing()
    b.set_incremental_packing()
    got = [b""] * B
    pos, rnd, windows, split = 0, 0, [], []
    while pos < max(lens):
        n = 7000 + 1152 * (rnd % 3)
        for s in range(B):
            a, e = min(pos, lens[s]), min(pos + n, lens[s])
            if e > a:
                b.append(s, xs[s][0, a:e], xs[s][1, a:e])
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", "3" if rnd % 3 == 1 else "0")
        monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "1" if rnd % 3 == 2 else "0")
        b.encode_available()
        windows.append(b.windows())
        split.append(bool(b.kernel_parts_ms()[0]))
        for s in range(B):
            got[s] += b.drain(s)
        pos += n
        rnd += 1
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "2")
    monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "0")
    b.finish()
    for s in range(B):
        got[s] += b.drain(s)
    assert got == want
    assert max(windows) > 1 and min(windows) == 1 and True in split and False in split, (windows, split)
    b.close()
    enc.close()


def test_backlog_small_buffers_and_bytes_in_place():
    """Drained only every third round, a stream's undrained rounds come with the next round's gather; a buffer that is too
    small returns -1 and takes nothing; drain_view hands out the same bytes in place"""
    sr, B = 44100, 8
    rng = np.random.default_rng(8901)
    enc = t.open_product(sr, dict(vbr_q=2))
    lens = [int(sr * 0.9) + 37 * s for s in range(B)]
    xs = [helpers.synth_stream(9970 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    plan = ragged_plan(rng, lens)
    cap = max(lens)
    want = s16_rounds(enc, lambda: lamehip.Batch(enc, B, cap), xs, plan)
    b = lamehip.Batch(enc, B, cap)
    b.set_device_packing()
    b.set_incremental_packing()
    b.lib.lamehip_batch_drain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    pos, owed, refused, views = [0] * B, [b""] * B, 0, 0
    for r, ns in enumerate(plan + [None]):
        if ns is None:
            b.finish()
        else:
            for s in range(B):
                b.append(s, xs[s][0, pos[s]:pos[s] + ns[s]], xs[s][1, pos[s]:pos[s] + ns[s]])
                pos[s] += ns[s]
            b.encode_available()
        for s in range(B):
            owed[s] += want[r][s]
        if r % 3 != 2 and ns is not None:
            continue
        for s in range(B):
            if len(owed[s]) > 1:
                small = C.create_string_buffer(len(owed[s]) - 1)
                assert b.lib.lamehip_batch_drain(b.b, s, small, len(small)) == -1
                refused += 1
            if s % 2:
                got = b.drain_view(s).tobytes()
                views += len(got) > 0
            else:
                got = b.drain(s)
            assert got == owed[s], "round %d stream %d" % (r, s)
            assert b.drain(s) == b"" and len(b.drain_view(s)) == 0
            owed[s] = b""
    assert refused > 8 and views > 4
    b.close()
    enc.close()


def test_conversion_and_replaygain_on_top_fed_from_a_tensor():
    """float32 at +/- 1.0 through append_device from a tensor on the same GPU, 48 -> 44.1 kHz and ReplayGain round by round
    on top of the switch, in a process of its own where torch takes the device first
    (tests/incremental_packing_child.py): bytes and radio gains of the same batch on the host packer"""
    child = os.path.join(helpers.ROOT, "tests", "incremental_packing_child.py")
    r = subprocess.run([sys.executable, child], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("incremental packing ok") == 1, r.stdout[-3000:]


def test_lifecycle_and_refusals():
    sr = 44100
    enc = t.open_product(sr, dict(brate=128))
    lib = enc.lib
    fn = lib.lamehip_batch_set_incremental_packing
    fn.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_last_error.restype = C.c_char_p
    x = helpers.synth_stream(9980, 6000, sr, 1.0 / 5)
    pl, pr = x[0].ctypes.data_as(C.c_void_p), x[1].ctypes.data_as(C.c_void_p)
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    # without device packing
    b = lamehip.Batch(enc, 1, 6000)
    assert fn(b.b, 1) == -1
    assert b"lamehip_batch_set_incremental_packing:" in lib.lamehip_last_error() and b"lamehip_batch_set_device_packing" in lib.lamehip_last_error()
    # with device tagging, and device tagging behind the switch
    b.set_device_packing()
    b.set_device_tagging()
    assert fn(b.b, 1) == -1
    assert b"lamehip_batch_set_device_tagging" in lib.lamehip_last_error()
    b.set_device_tagging(False)
    assert fn(b.b, 1) == 0
    with pytest.raises(RuntimeError, match="set_device_tagging"):
        b.set_device_tagging()
    # on = 0 restores the refusal of appends, with today's message
    assert fn(b.b, 0) == 0
    assert lib.lamehip_batch_append(b.b, 0, pl, pr, 100) == -1
    assert b"lamehip_batch_append:" in lib.lamehip_last_error() and b"packs on the device" in lib.lamehip_last_error()
    # after PCM was handed over
    b.set_pcm(0, x[0], x[1])
    assert fn(b.b, 1) == -1
    assert b"before any PCM" in lib.lamehip_last_error()
    b.close()
    # ReplayGain round by round: refused on a device-packed batch without the switch, accepted behind it
    b = lamehip.Batch(enc, 1, 6000)
    b.set_device_packing()
    with pytest.raises(RuntimeError, match="set_incremental_packing"):
        b.set_incremental_replaygain()
    b.set_incremental_packing()
    b.set_incremental_replaygain()
    b.close()
    # the whole life: rounds, finish, refusals until reset, the same bytes again
    b = lamehip.Batch(enc, 1, 6000)
    b.set_device_packing()
    b.set_incremental_packing()
    host = lamehip.Batch(enc, 1, 6000)
    host.append(0, x[0], x[1])
    host.encode_available()
    want = host.drain(0)
    host.finish()
    want += host.drain(0)
    host.close()
    for attempt in range(2):
        b.append(0, x[0, :2500], x[1, :2500])
        b.encode_available()
        out = b.drain(0)
        assert len(out) > 0 and b.drain_ms() > 0.0
        b.append(0, x[0, 2500:], x[1, 2500:])
        b.encode_available()
        out += b.drain(0)
        b.finish()
        assert b.drain_ms() > 0.0
        out += b.drain(0)
        assert out == want, attempt
        with pytest.raises(RuntimeError, match="finished"):
            b.append(0, x[0, :10], x[1, :10])
        with pytest.raises(RuntimeError, match="finished"):
            b.append_input(0, x[0, :10], x[1, :10])
        with pytest.raises(RuntimeError, match="finished"):
            b.encode_available()
        assert fn(b.b, 0) == -1         # (not on a batch that is being fed)
        b.reset()
        assert b.drain(0) == b""
    b.close()
    enc.close()
