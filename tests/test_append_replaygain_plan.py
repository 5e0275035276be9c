"""ReplayGain of an incremental batch without a device: the plan that follows the calls (csrc/lh_replaygain.c:
lh_gain_plan_call, lh_gain_plan_flush; a converting setting: the made counts of lh_rs_plan_call / lh_rs_plan_flush) against
the handle's calls restated in Python; the SOURCE of the kernel that resumes round by round (csrc/lh_gain.hip:
lh_gain_resume_kernel) run by the fiber emulator of tests/hipemu against the host twin bit for bit, windows and carry; and
the call plan and the twin as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import append_replaygain_support as sup
import gain_support as gs
import helpers
import resample_support as rsup

INC_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_gain_inc")
IDS = [s[0] for s in gs.SETTINGS]


@pytest.fixture(scope="module")
def lib():
    return sup.library()


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_gain_inc.so"], INC_DIR)
    e = C.CDLL(os.path.join(INC_DIR, "libhipemu_gain_inc.so"))
    e.lh_emu_gain_resume.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return e


# ---- the plan ----

@pytest.mark.parametrize("setting", gs.SETTINGS, ids=IDS)
def test_call_plan_equals_the_handles_calls(setting, lib):
    """every order of the lengths: call by call, and for the flush, the plan's blocks are the ones the handle hands to its
    analysis; the cursor counts what they add up to; the twin over all of them files the windows lh_rg_block files"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    for k, calls in enumerate(sup.call_orders(setting)):
        y = gs.heard(setting, gs.signal(setting, 900 + k, sum(calls), 0.5))
        hb, cp, at, blocks = sup.Calls(lib, setting), sup.CallPlan(lib, setting), 0, []
        for m in calls:
            first = len(hb.blocks)
            hb.feed(y[:, at:at + m])
            got = cp.call(m)
            assert got == hb.lengths(first), (name, k, m)
            if cp.rs is None:
                assert got == [fs] * (m // fs) + ([m % fs] if m % fs else [])
            assert cp.heard() == hb.fed
            at += m
            blocks += got
        first = len(hb.blocks)
        hb.flush()
        got = cp.flush()
        assert got == hb.lengths(first), (name, k, "flush")
        blocks += got
        assert cp.heard() == sum(blocks)
        x = hb.signal() if cp.rs is not None else y
        pairs, tenths = gs.eval_host(lib, rate_out, channels, blocks, x)
        hist, want = gs.block_by_block(lib, rate_out, channels, hb.blocks)
        assert gs.bins_of(lib, pairs, gs.window_of(rate_out)) == hist and tenths == want, (name, k)


@pytest.mark.parametrize("setting", gs.SETTINGS, ids=IDS)
def test_call_plan_of_the_empty_stream_is_the_flush(setting, lib):
    hb, cp = sup.Calls(lib, setting), sup.CallPlan(lib, setting)
    assert cp.call(0) == []
    assert cp.heard() == 0
    hb.flush()
    got = cp.flush()
    assert got == hb.lengths() and len(got) > 0 and cp.heard() == sum(got)


@pytest.mark.parametrize("setting", gs.SETTINGS, ids=IDS)
def test_whole_stream_plan_is_the_call_plan_fed_a_frame_per_call(setting, lib):
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    rs = rsup.resampler(lib, rate_in, rate_out) if rate_in != rate_out else None
    for n in gs.lengths_of(rate_in, rate_out, fs):
        cp, blocks = sup.CallPlan(lib, setting), []
        for at in range(0, n, fs):
            blocks += cp.call(min(fs, n - at))
        blocks += cp.flush()
        want, total = gs.plan(lib, rs, fs, n)
        assert blocks == [b for b in want if b > 0] and cp.heard() == total, (name, n)


def test_call_plan_refuses_what_no_stream_has(lib):
    cur = sup.LhGainCursor()
    lib.lh_gain_cursor_init(C.byref(cur))
    assert lib.lh_gain_plan_call(C.byref(cur), 1152, 1904, -1, None, 0) == -1
    assert lib.lh_gain_plan_call(C.byref(cur), 0, 1904, 5, None, 0) == -1
    assert lib.lh_gain_plan_flush(C.byref(cur), 0, 1904, None, 0) == -1
    assert cur.key() == (0, 0, 0)


# ---- the kernel's source under the emulator ----

def emu_rounds(emu, lib, rate, channels, fs, floats, pool, cap, streams, taps, matrix=(1.0, 0.0, 0.0, 1.0), one_plane=False):
    """lh_gain_resume_kernel round by round.  streams: [(row pair, rounds)], rounds: one (blocks, n) per round -- the round's
    block lengths (none: the stream is idle) and how far the row is real behind it; taps: the mapping of each round.  Returns
    (window sums per stream, float64 [windows, 2]; the carry array).  A round's output is NaN before, and NaN must remain
    behind every stream's windows; an idle stream's carry must come back as it was."""
    w = gs.window_of(rate)
    p = gs.LhGainParams()
    p.m[:] = matrix
    ky, kb = sup.filter_rows(rate)
    p.ky[:] = ky
    p.kb[:] = kb
    p.cap, p.window, p.fs, p.channels, p.one_plane = cap, w, fs, channels, int(one_plane)
    rows = pool.shape[0]
    carry = (sup.LhGainCarry * rows)()
    heard = {row: 0 for row, rounds in streams}
    wins = {row: [] for row, rounds in streams}
    for k in range(len(taps)):
        p.taps = taps[k]
        recs, tails, at, idle = [], [], 0, {}
        for row, rounds in streams:
            blocks, n = rounds[k]
            if sum(blocks) == 0:
                idle[row] = bytes(carry[row])
                continue
            recs.append(gs.LhGainStream(n, at, sum(blocks), row, 0, len(tails), len(blocks), 0))
            tails += blocks
            at += (heard[row] + sum(blocks)) // w - heard[row] // w + 1      # (one spare pair per stream: it must stay NaN)
        if not recs:
            continue
        arr = (gs.LhGainStream * len(recs))(*recs)
        tails_arr = (C.c_int * len(tails))(*tails)
        out = np.full((at, 2), np.nan, np.float64)
        assert emu.lh_emu_gain_resume(int(floats), C.byref(p), arr, len(recs), tails_arr, pool.ctypes.data, out.ctypes.data, carry) == 0
        for r in recs:
            nw = (heard[r.stream] + r.total) // w - heard[r.stream] // w
            assert not np.isnan(out[r.win_at:r.win_at + nw]).any(), "a window of the round is missing"
            assert np.isnan(out[r.win_at + nw]).all(), "written beyond the round's windows"
            wins[r.stream].append(out[r.win_at:r.win_at + nw].copy())
            heard[r.stream] += r.total
            assert carry[r.stream].heard == heard[r.stream]
        for row, before in idle.items():
            assert bytes(carry[row]) == before, "an idle stream's carry changed"
    return {row: (np.concatenate(v) if v else np.zeros((0, 2))) for row, v in wins.items()}, carry


# the mapping of the first filter's feedback per round: either one throughout, and switched from round to round
MAPPINGS = {"taps-across-lanes": [1] * 6, "lanes-0-and-1": [0] * 6, "switching": [1, 0, 0, 1, 0, 1], "switching-other-way": [0, 1, 1, 0, 1, 0]}

# per stream the calls of each of six rounds (input samples): rounds of fewer than 64 samples, rounds that end inside a
# window and inside a run of 64, a stream idle for a round (no call, or calls of nothing), a stream with one round only
ROUNDS = [
    [[1000, 1159], [], [9], [10, 11, 30], [2205, 1153, 64], [3000]],
    [[5], [20, 0, 40], [1152], [0], [1151, 1, 2204], [7]],
    [[], [], [4000, 1, 1], [], [], []],
]


def build_streams(lib, setting, seed):
    """the three streams of ROUNDS in a setting: per stream the input, what the analysis hears of it (float32 [2, n] without
    the flush's zeros; a converting setting: the converted signal, flush included), per round the blocks -- the flush joins
    the last round's, as lamehip_batch_finish has it -- and all blocks in one list"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    res = []
    for s, rounds in enumerate(ROUNDS):
        n = sum(sum(r) for r in rounds)
        assert n <= 0.3 * rate_in
        x = gs.signal(setting, seed + s, n, 1.0 if s != 1 else 0.25)
        y = gs.heard(setting, x)
        hb, cp, at, per_round = sup.Calls(lib, setting), sup.CallPlan(lib, setting), 0, []
        for calls in rounds:
            blocks = []
            for m in calls:
                hb.feed(y[:, at:at + m])
                blocks += cp.call(m)
                at += m
            per_round.append(blocks)
        hb.flush()
        per_round[-1] = per_round[-1] + cp.flush()
        assert [b for r in per_round for b in r] == hb.lengths()
        res.append((x, hb.signal() if cp.rs is not None else y, per_round))
    return res


def check_against_twin(lib, emu, setting, floats, pool, cap, built, extents, taps, **kw):
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    w = gs.window_of(rate_out)
    streams = [(s + 1, list(zip(built[s][2], extents[s]))) for s in range(len(built))]
    got, carry = emu_rounds(emu, lib, rate_out, channels, fs, floats, pool, cap, streams, taps, **kw)
    for s, (x, heard, per_round) in enumerate(built):
        blocks = [b for r in per_round for b in r]
        want, tenths = gs.eval_host(lib, rate_out, channels, blocks, heard)
        assert len(want) == sum(blocks) // w and len(want) > 0
        assert gs.same_doubles(got[s + 1], want), "stream %d" % s
        if channels == 1:
            assert (got[s + 1][:, 0] == got[s + 1][:, 1]).all()
        g = sup.twin_state(lib, rate_out, channels, blocks, heard)
        assert sup.carry_matches(carry[s + 1], g, channels, sum(blocks), len(want)) is None, "stream %d" % s
    assert bytes(carry[0]) == bytes(sup.LhGainCarry()), "the carry of a stream outside every round was written"


def extents_of(built, converting):
    """how far each stream's row is real behind each round: what was fed so far -- the flush's zeros are generated --, or,
    where the pool holds the converted signal, everything heard so far"""
    res = []
    for s, (x, heard, per_round) in enumerate(built):
        fed, heard_so_far, ext = 0, 0, []
        for k, blocks in enumerate(per_round):
            fed += sum(ROUNDS[s][k])
            heard_so_far += sum(blocks)
            ext.append(heard_so_far if converting else fed)
        res.append(ext)
    return res


@pytest.mark.parametrize("mapping", list(MAPPINGS), ids=list(MAPPINGS))
def test_resumed_kernel_matches_twin_s16_stereo_and_downmix(mapping, lib, emu):
    """the s16 path (the PCM matrix in the kernel): 44.1 kHz stereo, and mono downmixed from both planes at 0.6; the pool holds
    0x7fff beyond everything fed, in the rows of no stream, and -- stereo at the end -- where the flush's zeros are heard"""
    for setting, matrix in ((gs.SETTINGS[0], (1.0, 0.0, 0.0, 1.0)), (gs.SETTINGS[3], None)):
        name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
        if matrix is None:
            h = np.float32(0.5) * np.float32(scale)
            matrix = (h, h, 0.0, 0.0)
        built = build_streams(lib, setting, 70)
        cap = max(b[0].shape[1] for b in built) + 3
        pool = np.full((len(built) + 1, 2, cap), 0x7fff, np.int16)
        for s, (x, heard, per_round) in enumerate(built):
            pool[s + 1, :, :x.shape[1]] = x
        check_against_twin(lib, emu, setting, False, pool, cap, built, extents_of(built, False), MAPPINGS[mapping], matrix=matrix)


@pytest.mark.parametrize("mapping", list(MAPPINGS), ids=list(MAPPINGS))
def test_resumed_kernel_matches_twin_float_mono(mapping, lib, emu):
    """a float pool, mono: plane 0 stands for both sums; plane 1 and everything beyond what was fed is NaN"""
    setting = ("f32-32k-mono", 32000, 32000, 1, 1, 1.0, "f32unit", 1152)
    built = build_streams(lib, setting, 80)
    cap = max(b[0].shape[1] for b in built) + 5
    pool = np.full((len(built) + 1, 2, cap), np.nan, np.float32)
    for s, (x, heard, per_round) in enumerate(built):
        pool[s + 1, 0, :heard.shape[1]] = heard[0]
    check_against_twin(lib, emu, setting, True, pool, cap, built, extents_of(built, False), MAPPINGS[mapping], one_plane=True)


@pytest.mark.parametrize("mapping", ["taps-across-lanes", "switching-other-way"])
def test_resumed_kernel_matches_twin_converting(mapping, lib, emu):
    """48 -> 44.1 kHz: the float pool holds the converted signal, the rounds are the made counts of the conversion's call plan
    (blocks that make nothing dropped), the flush's blocks are in the pool; NaN beyond what each round has converted"""
    setting = gs.SETTINGS[5]
    built = build_streams(lib, setting, 90)
    cap = max(b[1].shape[1] for b in built) + 5
    pool = np.full((len(built) + 1, 2, cap), np.nan, np.float32)
    for s, (x, heard, per_round) in enumerate(built):
        pool[s + 1, :, :heard.shape[1]] = heard
        assert heard.shape[1] == sum(sum(r) for r in per_round)
    check_against_twin(lib, emu, setting, True, pool, cap, built, extents_of(built, True), MAPPINGS[mapping])


def test_call_plan_and_twin_under_sanitizers():
    """the stand-alone program (its own main; AddressSanitizer and UBSan linked in, nothing preloaded)"""
    helpers.locked_make(["gain_inc_host_check"], INC_DIR)
    r = subprocess.run([os.path.join(INC_DIR, "gain_inc_host_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
