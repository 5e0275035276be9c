"""Typed and device-resident appends of an incremental batch on the device (lamehip_batch_append_input / _append_input_device
/ _append_device, csrc/lh_ingest.hip: lh_append_kernel): every call gives the bytes of the reference entry point the batch's
sample type is named after, call by call; rounds fed from tensors on the same GPU, launches in windows and on changing
kernels, the staging arena's limits, the lifecycle and what stays refused."""
import ctypes as C
import functools
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

pytestmark = pytest.mark.gpu

# (id, sample type, rate, encoder settings, interleaved)
CASES = [
    ("f32unit-cbr128-js", PCM_F32_UNIT, 44100, dict(brate=128, mode=1), False),
    ("f32-vbr3", PCM_F32, 44100, dict(vbr_q=3), False),
    ("s32-mono96", PCM_S32, 44100, dict(brate=96, channels=1), False),
    ("f32unit-downmix", PCM_F32_UNIT, 44100, dict(vbr_q=2, mode=3), False),
    ("f32unit-scales", PCM_F32_UNIT, 44100, dict(brate=128, scale_left=0.7, scale_right=1.3), False),
    ("f32unit-22k-mpeg2", PCM_F32_UNIT, 22050, dict(brate=64), False),
    ("s16-interleaved", PCM_S16, 44100, dict(brate=128), True),
    ("f32unit-interleaved", PCM_F32_UNIT, 44100, dict(brate=128), True),
]
CHUNKS = [0, 1, 3, 575, 1152, 1153, 4000, 9000]


class EntryPoint:
    """one stream behind the entry point its sample type is named after, call by call: the compiled reference's where it was
    built (oracle/_ref), else this library's own handle call (as stream_bytes of tests/test_pcm_input_device.py)"""

    def __init__(self, stype, interleaved, sr, kw):
        self.kind, self.interleaved = psup.REF_KIND[(stype, interleaved)], interleaved
        self.buf = C.create_string_buffer(200000)
        if helpers.have_reference():
            self.ref, self.enc = helpers.Reference(), None
            self.h = t.open_reference(self.ref, sr, kw)
        else:
            self.ref, self.enc = None, t.open_product(sr, kw)
            self.fn = getattr(self.enc.lib, psup.HANDLE_CALL[self.kind])
            self.fn.restype = C.c_int

    def call(self, x):
        """x: [2, n] of the sample type"""
        n = x.shape[1]
        if self.interleaved:
            a, b = np.ascontiguousarray(x.T), None
        else:
            a, b = np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1])
        pa, pb = C.c_void_p(a.ctypes.data), None if b is None else C.c_void_p(b.ctypes.data)
        if self.ref:
            k = self.ref.lib.refh_encode_typed(self.h, self.kind, pa, pb, n, self.buf, len(self.buf))
        elif self.interleaved:
            k = self.fn(self.enc.h, pa, n, self.buf, len(self.buf))
        else:
            k = self.fn(self.enc.h, pa, pb, n, self.buf, len(self.buf))
        assert k >= 0
        return self.buf.raw[:k]

    def flush(self):
        if self.ref:
            k = self.ref.lib.refh_flush(self.h, self.buf, len(self.buf))
            self.ref.lib.refh_close(self.h)
        else:
            k = self.enc.lib.lame_encode_flush(self.enc.h, self.buf, len(self.buf))
            self.enc.close()
        assert k >= 0
        return self.buf.raw[:k]


def append_chunk(b, s, x, interleaved, mono):
    if interleaved:
        b.append_input(s, interleaved=np.ascontiguousarray(x.T))
    elif mono:
        b.append_input(s, np.ascontiguousarray(x[0]))
    else:
        b.append_input(s, np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1]))


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_appends_match_the_entry_point_call_by_call(case):
    """eight streams of 0.9 s + 37 s samples fed in ragged chunks (also empty ones), one encode_available per round: what
    every stream drains after a round is what the entry point returned for that stream's call of the round, and finish is
    its flush"""
    _, stype, sr, kw, interleaved = CASES[case]
    B = 8
    rng = np.random.default_rng(7700 + case)
    lens = [int(sr * 0.9) + 37 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9100 + 10 * case + s, lens[s], sr) for s in range(B)]
    eps = [EntryPoint(stype, interleaved, sr, kw) for _ in range(B)]
    enc = t.open_product(sr, kw)
    b = lamehip.Batch(enc, B, max(lens) + case % 4)
    if stype != PCM_S16:
        b.set_sample_type(stype)
    pos, rounds, total = [0] * B, 0, 0
    while any(pos[s] < lens[s] for s in range(B)):
        want = []
        for s in range(B):
            n = min(int(rng.choice(CHUNKS)), lens[s] - pos[s])
            x = xs[s][:, pos[s]:pos[s] + n]
            want.append(eps[s].call(x))
            append_chunk(b, s, x, interleaved, enc.channels == 1)
            pos[s] += n
        b.encode_available()
        for s in range(B):
            got = b.drain(s)
            assert got == want[s], "round %d stream %d" % (rounds, s)
            total += len(got)
        rounds += 1
    b.finish()
    for s in range(B):
        assert b.drain(s) == eps[s].flush(), "flush of stream %d" % s
    assert rounds > 3 and total > 8 * 5000
    if stype != PCM_S16:
        t.check_floats(b, enc, stype, xs)
    b.close()
    enc.close()


def one_shot(enc, stype, xs, cap):
    """pack(s) of a whole-stream batch of the same samples: set_input + encode"""
    b = lamehip.Batch(enc, len(xs), cap)
    if stype != PCM_S16:
        b.set_sample_type(stype)
    t.feed(b, xs, False, enc.channels == 1)
    b.encode()
    out = [b.pack(s) for s in range(len(xs))]
    b.close()
    return out


def drain_all(b, got, cap=1 << 20):
    for s in range(len(got)):
        got[s] += b.drain(s, cap)


def test_device_resident_appends_from_torch():
    """float32 streams held as one tensor on the GPU, in a process of its own where torch takes the device first
    (tests/append_input_child.py): rounds through append_device with ragged lengths (also 0), from [B, 2, T] tensors, views
    of larger ones and interleaved [B, T, 2]; then per stream through append_input with tensor slices, mixed with host
    arrays on alternate rounds -- the bytes and the floats of the one-shot typed batch"""
    child = os.path.join(helpers.ROOT, "tests", "append_input_child.py")
    r = subprocess.run([sys.executable, child], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("device-resident append ok") == 2, r.stdout[-3000:]


@pytest.mark.parametrize("switch", ["LAMEHIP_MID_WINDOW", "LAMEHIP_SPLIT_DENY"])
def test_typed_incremental_batch_in_windows_and_on_changing_kernels(switch, monkeypatch):
    """a typed incremental batch whose launches run in windows of frames every other round, or alternate between the split
    pipeline and the fused kernel: the bytes of the one-shot typed batch"""
    sr, B, stype = 44100, 4, PCM_F32_UNIT
    enc = t.open_product(sr, dict(brate=128))
    lens = [int(0.8 * sr) + 4111 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9300 + s, lens[s], sr) for s in range(B)]
    want = one_shot(enc, stype, xs, max(lens) + 3)
    b = lamehip.Batch(enc, B, max(lens) + 3)
    b.set_sample_type(stype)
    got = [b""] * B
    pos, rnd, seen = 0, 0, []
    while pos < max(lens):
        n = 7000 + 1152 * (rnd % 3)
        for s in range(B):
            a, e = min(pos, lens[s]), min(pos + n, lens[s])
            if e > a:
                b.append_input(s, xs[s][0, a:e], xs[s][1, a:e])
        monkeypatch.setenv(switch, ("3" if switch == "LAMEHIP_MID_WINDOW" else "1") if rnd % 2 else "0")
        b.encode_available()
        seen.append(b.windows() if switch == "LAMEHIP_MID_WINDOW" else bool(b.kernel_parts_ms()[0]))
        drain_all(b, got)
        pos += n
        rnd += 1
    monkeypatch.setenv(switch, "2" if switch == "LAMEHIP_MID_WINDOW" else "0")
    b.finish()
    drain_all(b, got)
    assert got == want
    if switch == "LAMEHIP_MID_WINDOW":
        assert max(seen) > 1 and min(seen) == 1, seen
    else:
        assert True in seen and False in seen, seen
    b.close()
    enc.close()


@functools.lru_cache(maxsize=None)
def arena_data():
    """two streams of 30 s (two seconds of signal, tiled) and a short one, float32, and the one-shot batch's bytes"""
    sr, stype = 44100, PCM_F32_UNIT
    n_long = 30 * sr
    two = [psup.typed_signal(stype, 9400 + s, 2 * sr, sr) for s in range(2)]
    xs = [np.ascontiguousarray(np.tile(x, (1, 15))[:, :n_long - 77 * s]) for s, x in enumerate(two)]
    xs.append(psup.typed_signal(stype, 9402, 9000, sr))
    enc = t.open_product(sr, dict(brate=128))
    want = one_shot(enc, stype, xs, n_long + 16)
    enc.close()
    return xs, want


def test_arena_limits_large_chunks_and_many_chunks():
    """one float32 chunk larger than a quarter of the staging arena (30 s: 10.6 MB of 16) is cut in pieces, and the next
    stream's does not fit beside it: what is staged leaves for HBM on the way (the first stream's floats are in the pool
    before any encode_available).  Then a round of more than 4096 chunks -- one sample each --, which crosses the chunk
    table's limit.  The bytes of the one-shot batch."""
    sr, stype = 44100, PCM_F32_UNIT
    xs, want = arena_data()
    enc = t.open_product(sr, dict(brate=128))
    b = lamehip.Batch(enc, 3, 30 * sr + 16)
    b.set_sample_type(stype)
    got = [b""] * 3
    b.append_input(0, xs[0][0], xs[0][1])
    assert b.converted(0).shape[1] == 0
    b.append_input(1, xs[1][0], xs[1][1])
    assert b.converted(0).shape[1] == xs[0].shape[1]            # flushed on the way
    singles = 4200
    for i in range(singles):
        b.append_input(2, xs[2][0, i:i + 1], xs[2][1, i:i + 1])
    b.encode_available()
    assert b.append_ms() > 0.0
    drain_all(b, got, 1 << 24)
    b.append_input(2, xs[2][0, singles:], xs[2][1, singles:])
    b.finish()
    drain_all(b, got, 1 << 24)
    for s in range(3):
        assert got[s] == want[s], s
    lib, cfg = psup.library(), enc.config()
    m = psup.matrix(lib, stype, cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r)
    assert psup.same_floats(b.converted(2), psup.host_ingest(lib, stype, m, xs[2][0], xs[2][1]))
    b.close()
    enc.close()


def test_lifecycle_and_refusals():
    """after finish the new calls fail until reset, then the same input gives the same bytes again; exceeding the capacity,
    a converting batch, a device-packed batch, a ReplayGain batch and stride 3 return -1 with a message that names the
    call, and the batch is usable afterwards"""
    lib = lamehip.load_library()
    sr, stype = 44100, PCM_F32_UNIT
    x = psup.typed_signal(stype, 9500, 6000, sr)
    enc = t.open_product(sr, dict(brate=128))
    want = one_shot(enc, stype, [x], 6000)
    b = lamehip.Batch(enc, 1, 6000)
    b.set_sample_type(stype)
    pl, pr = x[0].ctypes.data, x[1].ctypes.data
    lengths = (C.c_int * 1)(10)
    dev = b.pcm_device_ptr()                # (an address in HBM for the calls that are refused before they look at it)
    for attempt in range(2):
        b.append_input(0, x[0, :2500], x[1, :2500])
        # stride 3, and more than the capacity: refused, nothing counted
        assert lib.lamehip_batch_append_input(b.b, 0, pl, pr, 3, 100) == -1
        assert b"lamehip_batch_append_input:" in lib.lamehip_last_error() and b"stride 3" in lib.lamehip_last_error()
        assert lib.lamehip_batch_append_input_device(b.b, 0, dev, dev, 3, 100) == -1
        assert b"lamehip_batch_append_input_device:" in lib.lamehip_last_error()
        assert lib.lamehip_batch_append_device(b.b, dev, 0, 0, 3, lengths) == -1
        assert b"lamehip_batch_append_device:" in lib.lamehip_last_error()
        assert lib.lamehip_batch_append_input(b.b, 0, pl, pr, 1, 3501) == -1
        assert b"lamehip_batch_append_input:" in lib.lamehip_last_error() and b"capacity" in lib.lamehip_last_error()
        lengths[0] = 3501
        assert lib.lamehip_batch_append_device(b.b, dev, 0, 0, 1, lengths) == -1     # (refused before the address is looked at)
        assert b"lamehip_batch_append_device:" in lib.lamehip_last_error() and b"capacity" in lib.lamehip_last_error()
        lengths[0] = 10
        b.append_input(0, x[0, 2500:], x[1, 2500:])
        b.encode_available()
        out = b.drain(0)
        b.finish()
        out += b.drain(0)
        assert out == want[0], attempt
        for call in (lambda: b.append_input(0, x[0, :10], x[1, :10]), lambda: b.append_input(0, interleaved=x[:, :10].T.copy())):
            with pytest.raises(RuntimeError, match="finished"):
                call()
        assert lib.lamehip_batch_append_input_device(b.b, 0, dev, dev, 1, 10) == -1
        assert b"lamehip_batch_append_input_device:" in lib.lamehip_last_error() and b"finished" in lib.lamehip_last_error()
        assert lib.lamehip_batch_append_device(b.b, dev, 0, 0, 1, lengths) == -1
        assert b"lamehip_batch_append_device:" in lib.lamehip_last_error() and b"finished" in lib.lamehip_last_error()
        b.reset()
    b.close()
    # a device-packed batch and a ReplayGain batch: refused, and usable as whole-stream batches afterwards
    for what in ("packing", "replaygain"):
        b = lamehip.Batch(enc, 1, 6000)
        b.set_sample_type(stype)
        if what == "packing":
            b.set_device_packing()
        else:
            b.set_replaygain()
        dev = b.pcm_device_ptr()
        for name, (a0, a1) in (("lamehip_batch_append_input", (pl, pr)), ("lamehip_batch_append_input_device", (dev, dev))):
            assert getattr(lib, name)(b.b, 0, a0, a1, 1, 100) == -1
            assert name.encode() + b":" in lib.lamehip_last_error(), what
        assert lib.lamehip_batch_append_device(b.b, dev, 0, 0, 1, lengths) == -1
        assert b"lamehip_batch_append_device:" in lib.lamehip_last_error(), what
        b.set_input(0, x[0], x[1])
        b.encode()
        assert b.pack(0) == want[0], what
        b.close()
    enc.close()
    # a batch that converts the sample rate
    enc = t.open_product(48000, dict(brate=128), 44100)
    b = lamehip.Batch(enc, 1, 6000)
    b.set_device_resampling()
    b.set_sample_type(stype)
    dev = b.pcm_device_ptr()
    for name, (a0, a1) in (("lamehip_batch_append_input", (pl, pr)), ("lamehip_batch_append_input_device", (dev, dev))):
        assert getattr(lib, name)(b.b, 0, a0, a1, 1, 100) == -1
        assert name.encode() + b":" in lib.lamehip_last_error() and b"sample rate" in lib.lamehip_last_error()
    assert lib.lamehip_batch_append_device(b.b, dev, 0, 0, 1, lengths) == -1
    assert b"lamehip_batch_append_device:" in lib.lamehip_last_error() and b"sample rate" in lib.lamehip_last_error()
    b.set_input(0, x[0], x[1])
    b.encode()
    assert len(b.pack(0)) > 0
    b.close()
    enc.close()


def test_s16_batch_mixes_append_and_append_input():
    """an s16 batch fed through lamehip_batch_append and lamehip_batch_append_input in turn, planar and interleaved, also
    within one round: lame_encode_buffer / _interleaved either way, the bytes of the one-shot batch"""
    sr, B = 44100, 3
    enc = t.open_product(sr, dict(brate=128))
    lens = [int(0.7 * sr) + 501 * s for s in range(B)]
    xs = [helpers.synth_stream(9600 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    want = one_shot(enc, PCM_S16, xs, max(lens) + 1)
    b = lamehip.Batch(enc, B, max(lens) + 1)
    got = [b""] * B
    pos, rnd = 0, 0
    while pos < max(lens):
        n = 5000 + 777 * (rnd % 3)
        for s in range(B):
            a, m, e = min(pos, lens[s]), min(pos + n // 3, lens[s]), min(pos + n, lens[s])
            how = (rnd + s) % 3
            if how == 0:
                b.append(s, xs[s][0, a:m], xs[s][1, a:m])
                b.append_input(s, xs[s][0, m:e], xs[s][1, m:e])
            elif how == 1:
                b.append_input(s, interleaved=np.ascontiguousarray(xs[s][:, a:m].T))
                b.append(s, xs[s][0, m:e], xs[s][1, m:e])
            else:
                b.append_input(s, xs[s][0, a:e], xs[s][1, a:e])
        b.encode_available()
        drain_all(b, got)
        pos += n
        rnd += 1
    b.finish()
    drain_all(b, got)
    assert got == want
    b.close()
    enc.close()
