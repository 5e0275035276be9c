"""ReplayGain of an incremental batch on the device (lamehip_batch_set_incremental_replaygain; csrc/lh_gain.hip:
lh_gain_resume_kernel): after every round the window sums finished so far are the host twin's bit for bit over the blocks the
calls made so far, after finish the gain is lame_get_RadioGain of a handle fed the same calls, and the bytes are those of the
same batch without the switch; either mapping of the kernel and both sides of its threshold, idle streams, poisoned pools,
reset, whole-stream use before the first append, and what is refused."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import append_replaygain_support as sup
import gain_support as gs
import helpers
import lamehip

pytestmark = pytest.mark.gpu

IDS = [s[0] for s in gs.SETTINGS]


def lengths_of(setting):
    """the ragged batch of a setting, in input samples: nothing, less than a block's first piece, around a frame and a window,
    exactly the twelve call lengths, and 0.5 s and 0.7 s"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    w = gs.window_of(rate_out)
    return [0, 9, fs + 1, w + 10, 3 * fs, sum(sup.call_lengths(setting)), int(0.5 * rate_in), int(0.7 * rate_in)]


@functools.lru_cache(maxsize=None)
def case_data(k):
    """per setting, computed once and left alone: the streams, each stream's calls grouped into rounds of 0 to 3, and what a
    handle with findReplayGain returns for the same calls (bytes, gain)"""
    setting = gs.SETTINGS[k]
    xs = [gs.signal(setting, 9300 + 20 * k + s, n, 1.0 if s % 2 == 0 else 0.25) for s, n in enumerate(lengths_of(setting))]
    calls = [sup.calls_of(setting, s, x.shape[1]) for s, x in enumerate(xs)]
    rounds = [sup.into_rounds(c, 40 + 7 * k + s) for s, c in enumerate(calls)]
    handles = [sup.handle_calls(setting, x, c) for x, c in zip(xs, calls)]
    return xs, rounds, handles


def poison_pool(b, setting, nstreams, cap):
    """the whole input pool, through pcm_device_ptr: 0x7fff / NaN everywhere (gain_support.feed_batch_in_place's pattern)"""
    stype = setting[6]
    lib = b.lib
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.full((nstreams, 2, cap), np.nan, np.float32) if stype == "f32unit" else np.full((nstreams, 2, cap), 0x7fff, np.int16)
    assert lib.hipMemcpy(b.pcm_device_ptr(), host.ctypes.data, host.nbytes, 1) == 0     # 1 = hipMemcpyHostToDevice


def run_rounds(setting, xs, rounds, switch=True, poison=False, gains=None, torch_round=None, what=""):
    """the streams through an incremental batch, round by round; with the switch every round's windows and, at the end, the
    gains are checked.  Returns (bytes per stream, windows per stream, gain kernel time summed)"""
    lib = sup.library()
    enc = gs.open_handle(setting)
    B, cap = len(xs), max(x.shape[1] for x in xs) + 3
    b = sup.open_inc_batch(enc, setting, B, cap, switch)
    if poison:
        poison_pool(b, setting, B, cap)
    twins = [sup.Twin(lib, setting) for _ in range(B)]
    got, pos, keep, ms = [b""] * B, [0] * B, [], 0.0
    nrounds = max(len(r) for r in rounds)

    def check(s, final):
        want, tenths = twins[s].windows(b, enc, s, xs[s][:, :pos[s]])
        have = b.gain_windows(s)
        assert gs.same_doubles(have, want), "%s stream %d (%d of %d samples): window sums" % (what, s, pos[s], xs[s].shape[1])
        if final:
            assert b.radio_gain(s) == tenths, "%s stream %d: gain against the host twin" % (what, s)
        return have

    for k in range(nrounds):
        if torch_round is not None and k == torch_round[0]:
            ns = torch_round[1](b, xs, pos, [sum(r[k]) if k < len(r) else 0 for r in rounds])    # one call per stream from a tensor
            for s in range(B):
                if ns[s] > 0:
                    twins[s].call(ns[s])
                pos[s] += ns[s]
        else:
            for s in range(B):
                for i, m in enumerate(rounds[s][k] if k < len(rounds[s]) else []):
                    sup.append_call(b, setting, s, xs[s][:, pos[s]:pos[s] + m], (k + s + i) % 3, keep)
                    twins[s].call(m)
                    pos[s] += m
        b.encode_available()
        ms += b.gain_ms()
        for s in range(B):
            got[s] += b.drain(s)
            if switch:
                check(s, False)
        for d in keep:
            d.free()
        del keep[:]
    assert all(pos[s] == xs[s].shape[1] for s in range(B))
    if switch:
        with pytest.raises(RuntimeError, match="lamehip_batch_finish"):
            b.radio_gain(0)
    b.finish()
    ms += b.gain_ms()
    wins = []
    for s in range(B):
        got[s] += b.drain(s)
        twins[s].flush()
        if switch:
            wins.append(check(s, True))
            if gains is not None:
                assert b.radio_gain(s) == gains[s], "%s stream %d: gain against the handle" % (what, s)
    b.close()
    enc.close()
    return got, wins, ms


@pytest.mark.parametrize("k", range(len(gs.SETTINGS)), ids=IDS)
def test_rounds_match_host_twin_and_handle(k):
    """the ragged batch of every setting, cut into calls of the twelve lengths, 0 to 3 calls per stream and round, from host
    arrays (staged) and device arrays (resident) in turn: windows after every round, gains after finish, and the bytes of the
    same batch without the switch"""
    setting = gs.SETTINGS[k]
    xs, rounds, handles = case_data(k)
    got, wins, ms = run_rounds(setting, xs, rounds, gains=[h[1] for h in handles], what=setting[0])
    assert ms > 0.0
    assert len(set(h[1] for h in handles) - {0}) >= 2
    if setting[3] == 1:
        assert all((w[:, 0] == w[:, 1]).all() for w in wins)
    off, _, ms_off = run_rounds(setting, xs, rounds, switch=False)
    assert ms_off == 0.0
    assert got == off and sum(len(g) for g in got) > 10000


@pytest.mark.parametrize("k", [0, 5], ids=[IDS[0], IDS[5]])
def test_poisoned_pools_change_nothing(k):
    """the input pool filled with 0x7fff (NaN) before the first append: nothing at or beyond what a stream has been fed is read,
    by the analysis or by the converter in front of it -- the flush's zeros are generated"""
    setting = gs.SETTINGS[k]
    xs, rounds, handles = case_data(k)
    run_rounds(setting, xs, rounds, poison=True, gains=[h[1] for h in handles], what="poisoned " + setting[0])


def test_one_stream_cut_two_ways():
    """the same samples cut into calls two ways: each against its own twin and its own handle"""
    setting = gs.SETTINGS[0]
    x = gs.signal(setting, 9700, int(0.4 * 44100))
    for cut in ([x.shape[1]], sup.calls_of(setting, 3, x.shape[1])):
        rounds = [sup.into_rounds(cut, 5)]
        gain = sup.handle_calls(setting, x, cut)[1]
        got, wins, ms = run_rounds(setting, [x], rounds, gains=[gain], what="%d calls," % len(cut))
        assert len(wins[0]) >= 8 and gain != 0


@pytest.mark.parametrize("nstreams", [383, 384])
def test_either_side_of_the_mapping_threshold(nstreams):
    """LH_GN_TAPS_BELOW = 384 streams with work in a round: below it the first filter's feedback runs across the lanes of a row,
    from it on in lanes 0 and 1; 0.1 s per stream in three rounds, the last of them with work for one stream fewer -- so 384
    changes the mapping between rounds --, the first, the last and two streams in between against the host twin"""
    setting = gs.SETTINGS[0]
    lib = sup.library()
    base = [gs.signal(setting, 9900 + s, 4410 - 11 * s, 1.0 if s % 2 == 0 else 0.25) for s in range(4)]
    enc = gs.open_handle(setting)
    b = sup.open_inc_batch(enc, setting, nstreams, 4410)
    watched = (0, 129, 254, nstreams - 1)
    twins = {s: sup.Twin(lib, setting) for s in watched}
    for a, e in ((0, 1500), (1500, 1563), (1563, 4410)):
        for s in range(nstreams):
            x = base[s % 4]
            m = min(e, x.shape[1]) - a
            if e == 4410 and s == 7:
                continue                # (idle in the last round: its samples never come)
            b.append(s, x[0, a:a + m], x[1, a:a + m])
            if s in twins:
                twins[s].call(m)
        b.encode_available()
        assert b.gain_ms() > 0.0
        for s in watched:
            want, _ = twins[s].windows(b, enc, s, base[s % 4][:, :min(e, base[s % 4].shape[1])])
            assert gs.same_doubles(b.gain_windows(s), want), s
    b.finish()
    for s in watched:
        twins[s].flush()
        want, tenths = twins[s].windows(b, enc, s, base[s % 4])
        assert len(want) >= 2 and gs.same_doubles(b.gain_windows(s), want) and b.radio_gain(s) == tenths != 0, s
    b.close()
    enc.close()


def test_one_stream_of_67_has_work():
    """a round in which one stream of 67 is fed: the others' windows and state stay as they were, and their later rounds go on
    from there"""
    setting = gs.SETTINGS[0]
    lib = sup.library()
    xs = [gs.signal(setting, 9800 + (s % 3), 5000 + (s % 3)) for s in range(67)]
    enc = gs.open_handle(setting)
    b = sup.open_inc_batch(enc, setting, 67, 5100)
    twins = [sup.Twin(lib, setting) for _ in range(67)]
    pos = [0] * 67
    for k, who in enumerate((range(67), [41], range(67))):
        for s in who:
            m = (2300, 1200, xs[s].shape[1] - 2300 - (1200 if s == 41 else 0))[k]
            b.append(s, xs[s][0, pos[s]:pos[s] + m], xs[s][1, pos[s]:pos[s] + m])
            twins[s].call(m)
            pos[s] += m
        before = [b.gain_windows(s) for s in (0, 40, 66)] if k == 1 else None
        b.encode_available()
        if k == 1:
            assert b.gain_ms() > 0.0
            assert all(gs.same_doubles(b.gain_windows(s), w) for s, w in zip((0, 40, 66), before))
        for s in (0, 40, 41, 42, 66):
            want, _ = twins[s].windows(b, enc, s, xs[s][:, :pos[s]])
            assert gs.same_doubles(b.gain_windows(s), want), (k, s)
    b.finish()
    for s in range(67):
        twins[s].flush()
        want, tenths = twins[s].windows(b, enc, s, xs[s])
        assert gs.same_doubles(b.gain_windows(s), want) and b.radio_gain(s) == tenths, s
    b.close()
    enc.close()


def child(lanes):
    script = os.path.join(helpers.ROOT, "tests", "append_replaygain_child.py")
    env = dict(os.environ)
    env.pop("LAMEHIP_GAIN_LANES", None)
    if lanes is not None:
        env["LAMEHIP_GAIN_LANES"] = lanes
    r = subprocess.run([sys.executable, script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("incremental gain ok") == 1, r.stdout[-3000:]


@pytest.mark.parametrize("lanes", ["0", "1"], ids=["taps-across-lanes", "lanes-0-and-1"])
def test_mapping_forced_and_a_round_from_torch(lanes):
    """LAMEHIP_GAIN_LANES=0 / 1 in a process of its own, where torch takes the device first (tests/append_replaygain_child.py):
    setting 0's ragged batch, one round of it through append_device from a [B, 2, T] tensor -- either mapping whatever the
    round's size, the same windows and gains"""
    child(lanes)


def test_reset_and_again():
    """reset, then the same stream again: the same windows, the same gain, the same bytes; no gain in between"""
    setting = gs.SETTINGS[1]
    x = gs.signal(setting, 9750, 12000)
    enc = gs.open_handle(setting)
    b = sup.open_inc_batch(enc, setting, 2, 12000)
    runs = []
    for attempt in range(2):
        out = b""
        for a, e in ((0, 5000), (5000, 5007), (5007, 12000)):
            b.append(0, x[0, a:e], x[1, a:e])
            b.append_input(1, interleaved=np.ascontiguousarray(x[:, a:e].T))
            b.encode_available()
            out += b.drain(0)
        b.finish()
        out += b.drain(0)
        runs.append((b.gain_windows(0), b.gain_windows(1), b.radio_gain(0), b.radio_gain(1), out))
        b.reset()
        assert len(b.gain_windows(0)) == 0
        with pytest.raises(RuntimeError, match="lamehip_batch_finish"):
            b.radio_gain(0)
    assert len(runs[0][0]) >= 5 and runs[0][2] != 0
    assert gs.same_doubles(runs[0][0], runs[1][0]) and gs.same_doubles(runs[0][1], runs[1][1])
    assert runs[0][2:] == runs[1][2:]
    assert gs.same_doubles(runs[0][0], runs[0][1]) and runs[0][2] == runs[0][3]      # (append and append_input: the same call)
    b.close()
    enc.close()


@pytest.mark.parametrize("k", [0, 5], ids=[IDS[0], IDS[5]])
def test_whole_streams_before_any_append(k):
    """until the first append the batch is one with set_replaygain: whole streams through encode, the same windows, gains and
    tagged bytes"""
    setting = gs.SETTINGS[k]
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    xs = [gs.signal(setting, 9760 + s, n) for s, n in enumerate((int(0.3 * rate_in), fs + 1))]
    enc = gs.open_handle(setting, write_tag=True)
    res = []
    for inc in (False, True):
        b = gs.make_batch(enc, setting, len(xs), max(x.shape[1] for x in xs))
        if inc:
            if rate_in != rate_out:
                b.set_incremental_resampling()
            b.set_incremental_replaygain()
        else:
            b.set_replaygain()
        gs.feed_batch(b, setting, xs)
        b.encode()
        res.append([(b.gain_windows(s).tobytes(), b.radio_gain(s), b.pack_tagged(s)) for s in range(len(xs))])
        b.close()
    enc.close()
    assert res[0] == res[1] and res[0][0][1] != 0


def test_refusals():
    """every refusal of the switch and behind it, -1 and a lamehip_last_error() that names the call"""
    lib = lamehip.load_library()
    fn = lib.lamehip_batch_set_incremental_replaygain
    fn.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.lamehip_batch_append_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.lamehip_batch_radio_gain.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.lamehip_batch_set_replaygain.argtypes = [C.c_void_p, C.c_int]
    plain, conv = gs.SETTINGS[0], gs.SETTINGS[6]
    x = gs.signal(plain, 9770, 6000)
    pl, pr = x[0].ctypes.data, x[1].ctypes.data
    enc = gs.open_handle(plain)
    # after PCM, a length, the mirror or an append has been handed over
    for what in ("pcm", "length", "mirror", "append"):
        b = lamehip.Batch(enc, 1, 6000)
        if what == "pcm":
            b.set_pcm(0, x[0], x[1])
        elif what == "length":
            b.set_length(0, 100)
        elif what == "mirror":
            b.pcm_host()
        else:
            b.append(0, x[0, :100], x[1, :100])
        for on in (1, 0):
            assert fn(b.b, on) == -1, what
            assert b"lamehip_batch_set_incremental_replaygain:" in lib.lamehip_last_error(), what
        b.close()
    # a batch that packs on the device
    b = lamehip.Batch(enc, 1, 6000)
    b.set_device_packing()
    assert fn(b.b, 1) == -1
    assert b"lamehip_batch_set_incremental_replaygain:" in lib.lamehip_last_error() and b"lamehip_batch_set_device_packing" in lib.lamehip_last_error()
    b.close()
    # device packing switched on behind it: the appends stay refused
    b = lamehip.Batch(enc, 1, 6000)
    assert fn(b.b, 1) == 0
    b.set_device_packing()
    assert lib.lamehip_batch_append(b.b, 0, pl, pr, 100) == -1
    assert b"lamehip_batch_append:" in lib.lamehip_last_error() and b"packs on the device" in lib.lamehip_last_error()
    b.close()
    # on, then off again before the first append: the batch is as it was -- no gain, and set_replaygain's refusals are back
    b = lamehip.Batch(enc, 1, 6000)
    assert fn(b.b, 1) == 0 and fn(b.b, 1) == 0 and fn(b.b, 0) == 0
    b.append(0, x[0, :3000], x[1, :3000])
    b.encode_available()
    assert lib.lamehip_batch_get_gain_windows(b.b, 0, None, 0) == -1
    b.finish()
    tenths = C.c_int(7)
    assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(tenths)) == -1 and tenths.value == 7
    b.close()
    b = lamehip.Batch(enc, 1, 6000)
    b.set_replaygain()
    assert fn(b.b, 1) == 0 and fn(b.b, 0) == 0
    assert lib.lamehip_batch_append(b.b, 0, pl, pr, 100) == -1
    assert b"lamehip_batch_append:" in lib.lamehip_last_error() and b"lamehip_batch_set_replaygain" in lib.lamehip_last_error()
    b.close()
    # the gain before finish
    b = lamehip.Batch(enc, 1, 6000)
    assert fn(b.b, 1) == 0
    b.append(0, x[0, :3000], x[1, :3000])
    assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(tenths)) == -1
    assert b"lamehip_batch_radio_gain:" in lib.lamehip_last_error() and b"lamehip_batch_finish" in lib.lamehip_last_error()
    b.encode_available()
    assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(tenths)) == -1 and b"lamehip_batch_finish" in lib.lamehip_last_error()
    assert b.gain_windows(0).shape == (1, 2)
    # ... and set_replaygain on the incremental batch, as ever
    assert lib.lamehip_batch_set_replaygain(b.b, 1) == -1 and b"lamehip_batch_set_replaygain:" in lib.lamehip_last_error()
    b.finish()
    assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(tenths)) == 0
    b.close()
    enc.close()
    # a batch that converts the rate: only behind lamehip_batch_set_incremental_resampling
    enc = gs.open_handle(conv)
    for dev in (False, True):
        b = lamehip.Batch(enc, 1, 6000)
        if dev:
            b.set_device_resampling()
        assert fn(b.b, 1) == -1
        assert b"lamehip_batch_set_incremental_replaygain:" in lib.lamehip_last_error()
        assert b"lamehip_batch_set_incremental_resampling" in lib.lamehip_last_error()
        b.close()
    b = lamehip.Batch(enc, 1, 6000)
    b.set_device_resampling()
    b.set_incremental_resampling()
    assert fn(b.b, 1) == 0
    b.set_sample_type(lamehip.PCM_F32_UNIT)          # (before or after the sample type)
    f = (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    assert lib.lamehip_batch_append_input(b.b, 0, f[0].ctypes.data, f[1].ctypes.data, 1, 3000) == 0
    b.finish()
    assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(tenths)) == 0
    b.close()
    enc.close()


def test_stream_too_long_for_the_analysis(monkeypatch):
    """An append is refused when its stream, flushed right after the call, would be longer than the analysis takes: -1, the
    call named, nothing counted, the batch usable.  The real limit (0x7fffff00 samples) is beyond any pool a test would
    allocate, so the appends are told of a smaller one (LAMEHIP_INC_RG_MAX, a test aid): which calls fit follows from the plan."""
    lib = lamehip.load_library()
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    setting, limit = gs.SETTINGS[0], 8000
    plan = sup.library()

    def flushed(calls):
        cp = sup.CallPlan(plan, setting)
        for m in calls:
            cp.call(m)
        cp.flush()
        return cp.heard()

    assert flushed([3000]) <= limit < flushed([3000, 3000]) and flushed([3000, 1]) <= limit
    x = gs.signal(setting, 9780, 6000)
    enc = gs.open_handle(setting)
    monkeypatch.setenv("LAMEHIP_INC_RG_MAX", str(limit))
    b = sup.open_inc_batch(enc, setting, 2, 6000)
    monkeypatch.delenv("LAMEHIP_INC_RG_MAX")
    for s in range(2):
        b.append(s, x[0, :3000], x[1, :3000])
    assert lib.lamehip_batch_append(b.b, 0, x[0, 3000:].ctypes.data, x[1, 3000:].ctypes.data, 3000) == -1
    assert b"lamehip_batch_append:" in lib.lamehip_last_error() and b"ReplayGain" in lib.lamehip_last_error()
    for s in range(2):
        b.append(s, x[0, 3000:3001], x[1, 3000:3001])
    b.encode_available()
    b.finish()
    # the refused call counted nothing: stream 0, which met it, is stream 1
    assert gs.same_doubles(b.gain_windows(0), b.gain_windows(1)) and len(b.gain_windows(0)) == flushed([3000, 1]) // 2205
    assert b.radio_gain(0) == b.radio_gain(1) == sup.handle_calls(setting, x[:, :3001], [3000, 1])[1]
    assert b.drain(0) == b.drain(1)
    b.close()
    enc.close()


def test_set_replaygain_after_an_append_is_still_refused():
    """without the new switch nothing changed: lamehip_batch_set_replaygain on a batch fed with appends returns -1"""
    lib = lamehip.load_library()
    lib.lamehip_batch_set_replaygain.argtypes = [C.c_void_p, C.c_int]
    setting = gs.SETTINGS[0]
    x = gs.signal(setting, 9790, 2000)
    enc = gs.open_handle(setting)
    b = lamehip.Batch(enc, 1, 2000)
    b.append(0, x[0], x[1])
    assert lib.lamehip_batch_set_replaygain(b.b, 1) == -1
    assert b"lamehip_batch_set_replaygain:" in lib.lamehip_last_error() and b"incremental" in lib.lamehip_last_error()
    b.close()
    enc.close()
