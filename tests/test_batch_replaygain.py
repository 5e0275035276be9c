"""A batch's ReplayGain without a device: the host plan and the host twin (csrc/lh_replaygain.c: lh_gain_plan,
lh_gain_eval_host) against lh_rg_block / lh_rg_finish fed the blocks the handle API hands over -- and, where the compiled
reference is there, against its AnalyzeSamples / GetTitleGain --; the SOURCE of the device kernel (csrc/lh_gain.hip) run
by the fiber emulator of tests/hipemu against the host twin bit for bit; and the plan and the twin as a stand-alone
program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gain_support as gs
import helpers
import resample_support as rsup

GAIN_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_gain")


@pytest.fixture(scope="module")
def lib():
    return gs.library()


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_gain.so"], GAIN_DIR)
    e = C.CDLL(os.path.join(GAIN_DIR, "libhipemu_gain.so"))
    e.lh_emu_gain.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return e


@pytest.mark.parametrize("setting", gs.SETTINGS, ids=[s[0] for s in gs.SETTINGS])
def test_plan_and_twin_equal_block_by_block_analysis(setting, lib):
    """every length of the list: the plan's blocks are the handle's, and the twin's windows and gain are what lh_rg_block /
    lh_rg_finish (and the reference's analysis) make of the handle's blocks"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    ref = helpers.Reference().lib if helpers.have_reference() else None
    rs = rsup.resampler(lib, rate_in, rate_out) if rate_in != rate_out else None
    gains = set()
    for k, n in enumerate(gs.lengths_of(rate_in, rate_out, fs)):
        y = gs.heard(setting, gs.signal(setting, 500 + k, n, 1.0 if k % 2 == 0 else 0.25))
        hb = gs.HandleBlocks(lib, setting, y)
        blocks, total = gs.plan(lib, rs, fs, n)
        assert [b for b in blocks if b > 0] == [b.shape[1] for b in hb.blocks if b.shape[1] > 0], (name, n)
        assert total == sum(blocks)
        x = hb.signal() if rs is not None else y      # a converting batch hears the converted signal, flush included
        if rs is not None:
            assert x.shape[1] == total
        pairs, tenths = gs.eval_host(lib, rate_out, channels, blocks, x)
        got = gs.block_by_block(lib, rate_out, channels, hb.blocks, ref)
        w = gs.window_of(rate_out)
        assert len(pairs) == total // w
        assert gs.bins_of(lib, pairs, w) == got[0], (name, n)
        assert tenths == got[1], (name, n)
        assert tenths == lib.lh_gain_from_windows(pairs.ctypes.data, len(pairs), w)
        if ref is not None:
            assert tenths == got[2], (name, n)
        if channels == 1:
            assert (pairs[:, 0] == pairs[:, 1]).all()
        gains.add(tenths)
    assert len(gains - {0}) >= 2


def emu_run(emu, rate, channels, fs, floats, pool, cap, streams, trunk, matrix=(1.0, 0.0, 0.0, 1.0), one_plane=False, taps=1):
    """lh_gain_kernel under the emulator: the window sums of every stream of `streams' [(row pair, n, total, ntrunk, tail
    blocks)]; the output is NaN before, and NaN must remain behind every stream's windows"""
    w = gs.window_of(rate)
    p = gs.LhGainParams()
    p.m[:] = matrix
    ky, kb = filter_rows(rate)
    p.ky[:] = ky
    p.kb[:] = kb
    p.cap, p.window, p.fs, p.channels, p.one_plane = cap, w, fs, channels, int(one_plane)
    p.taps = taps
    recs, tail_list, at = [], [], 0
    for (s, n, total, ntrunk, tail) in streams:
        recs.append(gs.LhGainStream(n, at, total, s, ntrunk, len(tail_list), len(tail), 0))
        tail_list += tail
        at += total // w + 1                    # (one spare pair per stream: it must stay NaN)
    arr = (gs.LhGainStream * len(recs))(*recs)
    tails_arr = (C.c_int * max(len(tail_list), 1))(*tail_list)
    trunk_arr = (C.c_int * len(trunk))(*trunk) if trunk else None
    out = np.full((at, 2), np.nan, np.float64)
    assert emu.lh_emu_gain(int(floats), C.byref(p), arr, len(recs), trunk_arr, tails_arr, pool.ctypes.data, out.ctypes.data) == 0
    res = []
    for r in recs:
        nw = r.total // w
        assert np.isnan(out[r.win_at + nw]).all(), "written beyond the stream's windows"
        res.append(out[r.win_at:r.win_at + nw].copy())
    return res


def filter_rows(rate):
    """the rate's rows of csrc/lh_replaygain_tables.h, read from the header (the library does not export them)"""
    import re
    text = open(os.path.join(helpers.PKG, "csrc", "lh_replaygain_tables.h")).read()
    rows = {}
    for name, width in (("lh_rg_yule", 21), ("lh_rg_butter", 5)):
        body = text[text.index(name):]
        body = body[body.index("{") + 1:body.index("};")]
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        vals = [float(v.rstrip("fF")) for v in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?[fF]?|[-+]?\d+\.?(?:[eE][-+]?\d+)?[fF]?", body)]
        assert len(vals) == 9 * width, (name, len(vals))
        rows[name] = np.array(vals, np.float64).astype(np.float32).reshape(9, width)[gs.RATES.index(rate)]
    return list(rows["lh_rg_yule"]), list(rows["lh_rg_butter"])


@pytest.mark.parametrize("taps", [1, 0], ids=["taps-across-lanes", "lanes-0-and-1"])
def test_kernel_source_matches_host_twin_s16(taps, lib, emu):
    """three streams at 44.1 kHz stereo through the s16 path (the PCM matrix in the kernel), at most 0.3 s, one ending in
    0.25 s of digital silence -- its last windows are sums of squared subnormals --; the pool holds 0x7fff beyond every length"""
    setting = gs.SETTINGS[0]
    rate, fs, cap = 44100, 1152, 13300
    xs = [gs.signal(setting, 41, 13230), gs.signal(setting, 42, 2205 + 11025, 0.25), gs.signal(setting, 43, 1153)]
    xs[1][:, 2205:] = 0
    pool = np.full((4, 2, cap), 0x7fff, np.int16)
    streams, wants = [], []
    for s, x in enumerate(xs):
        n = x.shape[1]
        pool[s + 1, :, :n] = x                      # (row pairs 1..3: the stream index is not the list index)
        blocks, total = gs.plan(lib, None, fs, n)
        streams.append((s + 1, n, total, n // fs, blocks[n // fs:]))
        wants.append(gs.eval_host(lib, rate, 2, blocks, gs.heard(setting, x))[0])
    got = emu_run(emu, rate, 2, fs, False, pool, cap, streams, None, taps=taps)
    for s in range(3):
        assert len(wants[s]) > 0 and gs.same_doubles(got[s], wants[s]), "stream %d" % s
    late = wants[1][-1]
    assert 0 < late[0] < 1e-70 and 0 < late[1] < 1e-70      # every filter output in that window was subnormal or zero
    assert gs.same_doubles(got[1][-1:], wants[1][-1:])


@pytest.mark.parametrize("taps", [1, 0], ids=["taps-across-lanes", "lanes-0-and-1"])
def test_kernel_source_matches_host_twin_float_trunk_mono(taps, lib, emu):
    """a float pool behind a conversion plan (48 -> 44.1 kHz: the shared trunk and each stream's tail), mono: plane 0 stands
    for both sums, plane 1 and everything beyond a stream's length is NaN"""
    setting = ("f32-mono", 48000, 44100, 1, 1, 1.0, "f32unit", 1152)
    rate, fs = 44100, 1152
    rs = rsup.resampler(lib, 48000, 44100)
    lens = [14000, 1152 * 3, 700]
    plans = [rsup.plan(lib, rs, n) for n in lens]
    trunk = [b.made for b in plans[0][0][:plans[0][1]]]
    cap = max(p[2] for p in plans) + 7
    pool = np.full((3, 2, cap), np.nan, np.float32)
    streams, wants = [], []
    for s, n in enumerate(lens):
        blocks, ntrunk, conv = plans[s][0], plans[s][1], plans[s][2]
        made = [b.made for b in blocks]
        assert made[:ntrunk] == trunk[:ntrunk] and sum(made) == conv
        assert gs.plan(lib, rs, fs, n) == (made, conv)
        hb = gs.HandleBlocks(lib, setting, gs.heard(setting, gs.signal(setting, 60 + s, n, 0.5 if s else 1.0)))
        x = hb.signal()
        assert x.shape[1] == conv
        pool[s, 0, :conv] = x[0]
        streams.append((s, conv, conv, ntrunk, made[ntrunk:]))
        wants.append(gs.eval_host(lib, rate, 1, made, x)[0])
    got = emu_run(emu, rate, 1, fs, True, pool, cap, streams, trunk, taps=taps)
    for s in range(3):
        assert len(wants[s]) > 0 and gs.same_doubles(got[s], wants[s]), "stream %d" % s
        assert (got[s][:, 0] == got[s][:, 1]).all()


def test_host_plan_and_twin_under_sanitizers():
    """the stand-alone program (its own main; AddressSanitizer and UBSan linked in)"""
    helpers.locked_make(["gain_host_check"], GAIN_DIR)
    r = subprocess.run([os.path.join(GAIN_DIR, "gain_host_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
