"""A batch's statistics (lamehip_batch_set_statistics; csrc/lh_stats.hip: lh_stats_resume_kernel) on the GPU: every stream's
tables against the parse of that stream's own output bytes (tests/stats_support.py: header and side info only), which other
tests pin to the reference, and stream 0's against the parse of the golden bytes -- one-shot on both packers, launches in
windows, incremental rounds on both packers, slots that end and restart, reset, what is refused, poisoned device memory --,
and the handle API's block type tables for MPEG-2 / 2.5 streams.  Every check is integer equality."""
import ctypes as C

import numpy as np
import pytest

import helpers
import lamehip
import stats_support as ss

pytestmark = pytest.mark.gpu

NT = ss.NT


def golden(name):
    g, pcm = helpers.load_golden(name)
    keys, (channels, ngr) = ss.parse(g["mp3"].tobytes())
    ss.check_fixture_facts(name, keys, channels, ngr)
    return g, pcm, keys, channels, ngr


def tables_of(data, channels):
    keys, _ = ss.parse(data)
    return keys, ss.hist(keys, channels)


def assert_tables(got, want, what):
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), what


def one_shot(enc, xs, device, stats=True, cap=None):
    """a whole-stream batch over xs (None: a stream that is never declared); returns (batch, bytes per stream)"""
    b = lamehip.Batch(enc, len(xs), cap or max(x.shape[1] for x in xs if x is not None) + 16)
    if device:
        b.set_device_packing()
    if stats:
        b.set_statistics()
    for s, x in enumerate(xs):
        if x is not None:
            b.set_pcm(s, x[0], x[1])
    b.encode()
    out = [b"" if x is None else (b.get_bytes(s) if device else b.pack(s)) for s, x in enumerate(xs)]
    return b, out


def handle_tables(g, pcm):
    """the six getters of the handle API behind a whole stream"""
    enc = lamehip.Encoder(**helpers.golden_encoder_kwargs(g))
    out = b""
    for a in range(0, pcm.shape[1], 5000):
        out += enc.encode(pcm[0][a:a + 5000], pcm[1][a:a + 5000])
    out += enc.flush()
    res = {}
    for name, n in (("bitrate_kbps", 14), ("bitrate_hist", 14), ("stereo_mode_hist", 4), ("bitrate_stereo_mode_hist", 56),
                    ("block_type_hist", 6), ("bitrate_block_type_hist", 84)):
        a = (C.c_int * n)()
        f = getattr(enc.lib, "lame_" + name)
        f.restype, f.argtypes = None, [C.c_void_p, C.c_void_p]
        f(enc.h, a)
        res[name] = np.array(list(a), np.int32)
    enc.close()
    return out, res


def shaped_getters(b, s):
    """the five reference-shaped getters and bitrate_kbps through the C entry points"""
    res = {}
    for name, n in (("bitrate_hist", 14), ("stereo_mode_hist", 4), ("bitrate_stereo_mode_hist", 56), ("block_type_hist", 6),
                    ("bitrate_block_type_hist", 84)):
        a = (C.c_int * n)()
        f = getattr(b.lib, "lamehip_batch_" + name)
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        assert f(b.b, s, a) == 0, lamehip.last_error()
        res[name] = np.array(list(a), np.int32)
    res["bitrate_kbps"] = b.bitrate_kbps()
    return res


# ---- 1. one-shot ----

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(ss.FIXTURES))
def test_one_shot_batch(name, device):
    g, pcm, gkeys, channels, ngr = golden(name)
    n, fs = pcm.shape[1], 576 * ngr
    xs = [pcm, pcm[:, :fs], pcm[:, :n // 2], None, pcm[:, :n // 3 + 17], pcm[:, 5:2 * n // 3]]
    enc = lamehip.Encoder(**helpers.golden_encoder_kwargs(g))
    b, out = one_shot(enc, xs, device)
    assert b.stats_ms() > 0.0
    assert out[0] == g["mp3"].tobytes()
    every = b.statistics_all()
    for s in range(len(xs)):
        keys, want = tables_of(out[s], channels)
        got = b.statistics(s)
        assert_tables(got, want, (name, s))
        assert (every[s] == ss.flat(*want)).all()
        assert b.frames(s) == len(keys) == got[0][15][4]
        sh = shaped_getters(b, s)
        assert (sh["bitrate_hist"] == got[0][1:15, 4]).all() and (b.bitrate_hist(s) == sh["bitrate_hist"]).all()
        assert (sh["stereo_mode_hist"] == got[0][15, :4]).all() and (b.stereo_mode_hist(s) == sh["stereo_mode_hist"]).all()
        assert (sh["bitrate_stereo_mode_hist"].reshape(14, 4) == got[0][1:15, :4]).all()
        assert (sh["block_type_hist"] == got[1][15]).all() and (b.block_type_hist(s) == sh["block_type_hist"]).all()
        assert (sh["bitrate_block_type_hist"].reshape(14, 6) == got[1][1:15]).all()
        kbps = [ss.KBPS[1 if ngr == 2 else 0][i] for i in range(1, 15)]
        assert list(sh["bitrate_kbps"]) == kbps
        if keys:
            assert b.average_kbps(s) == sum(kbps[k[0] - 1] for k in keys) / len(keys)
    assert b.frames(3) == 0 and not every[3].any() and b.average_kbps(3) == 0.0
    assert_tables(b.statistics(0), ss.hist(gkeys, channels), name)
    # the handle API, run on stream 0
    hout, h = handle_tables(g, pcm)
    assert hout == out[0]
    sh = shaped_getters(b, 0)
    for k in sh:
        assert (sh[k] == h[k]).all(), k
    b.close()
    enc.close()


# ---- 2. launches in windows ----

def test_launch_in_windows(monkeypatch):
    """streams of NT - 1, NT, NT + 1 and 2 NT + 1 frames at CBR 128, the launch whole and in windows of 64 frames"""
    sr = 44100
    enc = lamehip.Encoder(sr, 128)
    counts = [NT - 1, NT, NT + 1, 2 * NT + 1]
    long = helpers.synth_stream(4242, (2 * NT + 1) * 1152, sr, 1.0 / 4)
    xs = []
    for s, k in enumerate(counts):
        n = (k - 2) * 1152
        while enc.lib.lh_total_frames_fs(C.c_long(n), 1152) < k:
            n += 100
        assert enc.lib.lh_total_frames_fs(C.c_long(n), 1152) == k
        xs.append(np.ascontiguousarray(long[:, 300 * s:300 * s + n]))
    res = []
    for window in ("0", "64"):
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", window)
        b, out = one_shot(enc, xs, True)
        assert (b.windows() > 1) == (window != "0") and b.kernel_parts_ms()[0]
        for s, k in enumerate(counts):
            keys, want = tables_of(out[s], 2)
            assert len(keys) == k == b.frames(s)
            assert_tables(b.statistics(s), want, (window, s))
        res.append((out, b.statistics_all()))
        b.close()
    assert res[0][0] == res[1][0] and (res[0][1] == res[1][1]).all()
    enc.close()


# ---- 3. incremental rounds ----

def frames_complete(fed, ngr):
    """frames an encoder has made of `fed' samples before any flush: it starts with 528 samples of delay in its buffer and
    makes a frame whenever it holds 1024 + 576 granules - 272 (reference lame.c: mf_samples_to_encode, mf_needed)"""
    fs, need = 576 * ngr, 1024 + 576 * ngr - 272
    return (fed + 528 - need) // fs + 1 if fed + 528 >= need else 0


def incremental_batch(enc, B, cap, device):
    b = lamehip.Batch(enc, B, cap)
    if device:
        b.set_device_packing()
        b.set_incremental_packing()
        b.set_incremental_tagging()
    b.set_statistics()
    return b


@pytest.mark.parametrize("device", [False, True], ids=["host", "packing+tagging"])
@pytest.mark.parametrize("name", ["vbr2_js_44k", "abr56_js_22k_lsf"])
def test_incremental_rounds(name, device):
    g, pcm, gkeys, channels, ngr = golden(name)
    n = pcm.shape[1]
    xs = [pcm, pcm[:, :n // 2], pcm[:, 11:n // 3 + 11]]
    B = len(xs)
    enc = lamehip.Encoder(**helpers.golden_encoder_kwargs(g))
    b = incremental_batch(enc, B, n + 16, device)
    rng = np.random.default_rng(77)
    pos, out, snaps, made = [0] * B, [b""] * B, [], 0
    rnd = 0
    while any(pos[s] < xs[s].shape[1] for s in range(B)):
        for s in range(B):
            # (empty rounds, rounds shorter than a frame, rounds of several frames)
            k = [0, 100, 0, 700, 5000, 9000][(rnd + s) % 6] if rnd % 4 != 3 else 0
            k = min(k + int(rng.integers(0, 50)) * (k > 0), xs[s].shape[1] - pos[s])
            b.append(s, xs[s][0, pos[s]:pos[s] + k], xs[s][1, pos[s]:pos[s] + k])
            pos[s] += k
        got = b.encode_available()
        assert (b.stats_ms() > 0.0) == (got > 0)
        made += got
        snaps.append((list(pos), b.statistics_all().copy()))
        for s in range(B):
            out[s] += b.drain(s)
        rnd += 1
    assert sum(frames_complete(pos[s], ngr) for s in range(B)) == made and len(snaps) > 8
    b.finish()
    assert b.stats_ms() > 0.0
    for s in range(B):
        out[s] += b.drain(s)
    assert out[0] == g["mp3"].tobytes()
    keys = [ss.parse(out[s])[0] for s in range(B)]
    for fed, tables in snaps:
        for s in range(B):
            done = frames_complete(fed[s], ngr)
            assert (tables[s] == ss.flat(*ss.hist(keys[s][:done], channels))).all(), (fed, s)
    for s in range(B):
        got = b.statistics(s)
        assert_tables(got, ss.hist(keys[s], channels), s)
        assert b.frames(s) == len(keys[s]) == got[0][15][4]
    assert_tables(b.statistics(0), ss.hist(gkeys, channels), name)
    b.close()
    enc.close()


# ---- 4. slots ----

@pytest.mark.parametrize("device", [False, True], ids=["host", "packing+tagging"])
def test_slots_end_and_restart(device):
    g, pcm, gkeys, channels, ngr = golden("vbr2_js_44k")
    n = pcm.shape[1]
    first = [pcm, pcm[:, :20000], pcm[:, 7:n - 3000]]
    second = pcm[:, 9000:9000 + 26001]
    enc = lamehip.Encoder(**helpers.golden_encoder_kwargs(g))
    b = incremental_batch(enc, 3, n + 16, device)
    out, zeros = [b"", b"", b""], (np.zeros((16, 5), np.int32), np.zeros((16, 6), np.int32))

    def feed(a, e, streams):
        for s in streams:
            x = first[s]
            b.append(s, x[0, min(a, x.shape[1]):min(e, x.shape[1])], x[1, min(a, x.shape[1]):min(e, x.shape[1])])
        b.encode_available()
        for s in range(3):
            out[s] += b.drain(s)

    feed(0, 12000, (0, 1, 2))
    feed(12000, 20000, (0, 1, 2))
    b.end_stream(1)
    feed(20000, 30000, (0, 2))
    assert b.stream_ended(1)
    ended = tables_of(out[1], channels)
    assert len(ended[0]) == b.frames(1) > 10
    assert_tables(b.statistics(1), ended[1], "ended stream")
    feed(30000, 41000, (0, 2))
    assert_tables(b.statistics(1), ended[1], "ended stream, a round later")
    mid = [b.statistics(s) for s in (0, 2)]
    b.restart_stream(1)
    assert_tables(b.statistics(1), zeros, "restarted slot")
    for k, s in enumerate((0, 2)):
        assert_tables(b.statistics(s), mid[k], "neighbour %d of the restarted slot" % s)
    old, out[1] = out[1], b""
    b.append(1, second[0], second[1])
    feed(41000, 52000, (0, 2))
    assert 0 < b.statistics(1)[0][15][4] == frames_complete(second.shape[1], ngr)
    feed(52000, n, (0, 2))
    b.finish()
    for s in range(3):
        out[s] += b.drain(s)
    assert out[0] == g["mp3"].tobytes() and out[1] != old
    for s in range(3):
        keys, want = tables_of(out[s], channels)
        assert_tables(b.statistics(s), want, "stream %d behind finish" % s)
        assert b.frames(s) == len(keys)
    assert_tables(b.statistics(0), ss.hist(gkeys, channels), "stream 0")
    b.close()
    enc.close()


# ---- 5. reset ----

def test_reset_gives_zeros_and_a_second_run_the_same_tables():
    g, pcm, gkeys, channels, ngr = golden("mono_vbr2_44k")
    enc = lamehip.Encoder(**helpers.golden_encoder_kwargs(g))
    want = ss.flat(*ss.hist(gkeys, channels))
    # one-shot
    b, out = one_shot(enc, [pcm, pcm[:, :9999]], True)
    t1 = b.statistics_all().copy()
    assert (t1[0] == want).all() and t1[1].any()
    b.reset()
    assert not b.statistics_all().any()
    b.encode()
    assert (b.statistics_all() == t1).all()
    b.encode()                                              # (and every encode counts from zero)
    assert (b.statistics_all() == t1).all()
    b.close()
    # incremental
    b = incremental_batch(enc, 2, pcm.shape[1] + 16, True)
    for run in range(2):
        for a in range(0, pcm.shape[1], 15000):
            b.append(0, pcm[0, a:a + 15000])
            b.append(1, pcm[0, a:min(a + 15000, 9999)])
            b.encode_available()
        b.finish()
        assert (b.statistics_all() == t1).all(), run
        b.reset()
        assert not b.statistics_all().any()
    b.close()
    enc.close()


# ---- 6. refusals ----

def test_refusals_and_the_switch_off():
    g, pcm, gkeys, channels, ngr = golden("cbr192_st_44k")
    enc = lamehip.Encoder(**helpers.golden_encoder_kwargs(g))
    xs = [pcm, pcm[:, :7000]]
    off, out_off = one_shot(enc, xs, True, stats=False)
    on, out_on = one_shot(enc, xs, True)
    assert off.stats_ms() == 0.0 and on.stats_ms() > 0.0 and out_off == out_on
    for call in (lambda: off.statistics(0), off.statistics_all, lambda: off.bitrate_hist(0), lambda: off.stereo_mode_hist(0),
                 lambda: off.block_type_hist(0), off.bitrate_kbps, lambda: off.average_kbps(0)):
        with pytest.raises(RuntimeError, match=r"lamehip_batch_\w+: the batch keeps no statistics \(lamehip_batch_set_statistics\)"):
            call()
    buf = (C.c_int * 84)()
    for name in ("bitrate_stereo_mode_hist", "bitrate_block_type_hist"):
        f = getattr(off.lib, "lamehip_batch_" + name)
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        assert f(off.b, 0, buf) == -1 and lamehip.last_error().startswith("lamehip_batch_" + name + ":")
        assert f(on.b, 2, buf) == -1 and lamehip.last_error() == "lamehip_batch_%s: no stream 2 (the batch has 2)" % name
    for s in (-1, 2):
        for call in (on.statistics, on.bitrate_hist, on.stereo_mode_hist, on.block_type_hist):
            with pytest.raises(RuntimeError, match=r"lamehip_batch_\w+: no stream %d \(the batch has 2\)" % s):
                call(s)
    # the switch once PCM, a length or an append has been handed over
    for b in (off, on):
        with pytest.raises(RuntimeError, match="lamehip_batch_set_statistics: only before any PCM is handed over"):
            b.set_statistics()
    off.close()
    on.close()
    for hand_over in ("pcm", "length", "append"):
        b = lamehip.Batch(enc, 1, 5000)
        if hand_over == "pcm":
            b.set_pcm(0, pcm[0, :100], pcm[1, :100])
        elif hand_over == "length":
            b.set_length(0, 100)
        else:
            b.append(0, pcm[0, :100], pcm[1, :100])
        with pytest.raises(RuntimeError, match="lamehip_batch_set_statistics: only before any PCM is handed over"):
            b.set_statistics()
        b.close()
    # on and off again before anything is handed over
    b = lamehip.Batch(enc, 1, 5000)
    b.set_statistics()
    b.set_statistics(False)
    with pytest.raises(RuntimeError, match="keeps no statistics"):
        b.statistics(0)
    b.close()
    enc.close()


# ---- 7. poisoned device memory ----

@pytest.mark.parametrize("name", ["mono_vbr2_44k", "abr56_js_22k_lsf", "cbr16_js_8k_lsf"])
def test_poisoned_pools(name):
    """registers, LDS and scratch poisoned before the launch (tests/gpu_tools/lh_poison.hip), and the memory the batch's pools
    are made of filled with 0xA5 before they are allocated: the granules and channels the streams do not have hold garbage"""
    import test_gpu_parity as tgp
    g, pcm, gkeys, channels, ngr = golden(name)
    enc = lamehip.Encoder(**helpers.golden_encoder_kwargs(g))
    lib = enc.lib
    lib.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
    lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    for device in (False, True):
        size = 3 * (int(g["nframes"]) + 1024) * 4928
        blocks = []
        for k in range(3):
            p = C.c_void_p()
            assert lib.hipMalloc(C.byref(p), size >> k) == 0
            assert lib.hipMemset(p, 0xA5, size >> k) == 0
            blocks.append(p)
        assert lib.hipDeviceSynchronize() == 0
        for p in blocks:
            assert lib.hipFree(p) == 0
        b = lamehip.Batch(enc, 2, pcm.shape[1] + 16)
        if device:
            b.set_device_packing()
        b.set_statistics()
        b.set_pcm(0, pcm[0], pcm[1])
        b.set_pcm(1, pcm[0, :pcm.shape[1] // 2], pcm[1, :pcm.shape[1] // 2])
        assert tgp._poison_tool().lamehip_test_poison(C.c_uint(0xA5A5A5A5)) == 0
        b.encode()
        out = [b.get_bytes(s) if device else b.pack(s) for s in range(2)]
        assert out[0] == g["mp3"].tobytes()
        assert_tables(b.statistics(0), ss.hist(gkeys, channels), name)
        assert_tables(b.statistics(1), tables_of(out[1], channels)[1], name)
        b.close()
    enc.close()


# ---- 8. the handle API, MPEG-2 / 2.5 ----

@pytest.mark.parametrize("name", ss.LSF)
def test_handle_counts_one_granule_per_lsf_frame(name):
    g, pcm, gkeys, channels, ngr = golden(name)
    out, h = handle_tables(g, pcm)
    assert out == g["mp3"].tobytes()
    mode, block = ss.hist(gkeys, channels)
    assert (h["block_type_hist"] == block[15]).all()
    assert h["block_type_hist"][5] == len(gkeys) * channels
    assert (h["bitrate_block_type_hist"].reshape(14, 6) == block[1:15]).all()
    assert (h["bitrate_hist"] == mode[1:15, 4]).all() and (h["stereo_mode_hist"] == mode[15, :4]).all()


@pytest.mark.parametrize("name,rate,kw", [("abr56_js_22k_lsf", 22050, dict(abr=56)), ("cbr16_js_8k_lsf", 8000, dict(brate=16))])
def test_handle_counts_what_the_live_reference_counts(name, rate, kw, reference):
    import test_resample as T
    import test_stats
    g, pcm, gkeys, channels, ngr = golden(name)
    rlib = reference.lib
    rlib.refh_gfp.restype = C.c_void_p
    rh = T.open_reference(reference, rate, kw, 0)
    rg = C.c_void_p(rlib.refh_gfp(rh))
    enc = T.open_product(rate, kw, 0, require_device=True)
    buf = C.create_string_buffer(100000)
    for a in range(0, pcm.shape[1], 5000):
        l, r = np.ascontiguousarray(pcm[0][a:a + 5000]), np.ascontiguousarray(pcm[1][a:a + 5000])
        k = rlib.refh_encode(rh, l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), len(l), buf, len(buf))
        assert enc.encode(l, r) == buf.raw[:k]
    k = rlib.refh_flush(rh, buf, len(buf))
    assert enc.flush() == buf.raw[:k]
    got, want = test_stats.snapshot(enc.lib, enc.h), test_stats.snapshot(rlib, rg)
    assert got == want
    assert got[4] == list(ss.hist(gkeys, channels)[1][15])
    rlib.refh_close(rh)
    enc.close()
