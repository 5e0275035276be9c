"""The conversion plan of an incremental batch (lamehip_batch_set_incremental_resampling; csrc/lh_resample.c:
lh_rs_plan_call, lh_rs_plan_flush, lh_rs_block_tiles): where the reference cuts its blocks depends on how
lame_encode_buffer is called, so the plan follows the calls from a cursor per stream, and a block goes to the device in
tiles whose input span fits the kernel's LDS.  Checked against lh_rs_block driven call by call; the device kernel's SOURCE
(csrc/lh_resample_dev.hip: lh_resample_tiles_kernel) and the as-it-is append (csrc/lh_ingest.hip) run under the fiber
emulator of tests/hipemu; the plan functions once more as a program of their own under the sanitizers.  Everything is
compared bit for bit."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import append_resample_support as asup
import helpers
import lamehip
import pcm_input_support as psup
import resample_support as rsup
import test_append_input as tai
from lamehip import PCM_F32_UNIT, PCM_S16, PCM_S32
from resample_support import FS, MFN

PAIRS = [(48000, 44100), (44100, 48000), (96000, 32000), (44100, 32000), (32000, 44100), (8000, 32000)]
PAIR_IDS = ["%d-%d" % p for p in PAIRS]
SIZES = [0, 1, 3, 33, 575, 1151, 1152, 1153, 4000, 9000, 50000]


@pytest.fixture(scope="module")
def lib():
    return asup.library()


def patterns(rate_in):
    """call patterns of about 20 calls drawn from SIZES with a fixed seed; the second starts with the large calls"""
    rng = np.random.default_rng(5100 + rate_in)
    return [[int(v) for v in rng.choice(SIZES, 20)], [50000, 9000, 0] + [int(v) for v in rng.choice(SIZES, 17)]]


def noise(seed, n):
    return (np.random.default_rng(seed).standard_normal((2, n)) * 9000).astype(np.float32)


def keys(blocks):
    return [b.key() for b in blocks]


@pytest.mark.parametrize("rate_in,rate_out", PAIRS, ids=PAIR_IDS)
def test_plan_follows_lh_rs_block_call_by_call(rate_in, rate_out, lib):
    """after every call: the call's blocks (in_at, out_at, start, len, made) and the cursor (clock, consumption, converted
    count, mf_size, frames) are those of lh_rs_block driven through the same call; then the flush from the final cursor is
    the handle's flush loop -- blocks, converted length, frames, padding"""
    rs = rsup.resampler(lib, rate_in, rate_out)
    for pi, pattern in enumerate(patterns(rate_in)):
        chain, cur = asup.HostChain(lib, rate_in, rate_out, channels=1), asup.cursor(lib)
        for ci, m in enumerate(pattern):
            want = chain.call(noise(100 * pi + ci, m))
            got = asup.plan_call(lib, rs, cur, m)
            assert keys(got) == want, "pattern %d call %d (%d samples)" % (pi, ci, m)
            assert asup.cursor_key(cur) == chain.state(), "pattern %d call %d" % (pi, ci)
            assert cur.in_at == sum(pattern[:ci + 1])
        want, want_padding = chain.flush()
        got, padding = asup.plan_flush(lib, rs, cur)
        assert keys(got) == want and padding == want_padding, "pattern %d: flush" % pi
        assert asup.cursor_key(cur) == chain.state()
        assert cur.nblk == len(chain.blocks)


@pytest.mark.parametrize("rate_in,rate_out", PAIRS, ids=PAIR_IDS)
def test_calls_of_a_frame_give_the_whole_stream_plan(rate_in, rate_out, lib):
    """calls of 1152, the remainder, then the flush: exactly lh_rs_plan's blocks, length, frames and padding"""
    rs = rsup.resampler(lib, rate_in, rate_out)
    for n in [0, 1, 16, 1151, 1152, 1153, 2304, 5000, rate_in // 2 + 13]:
        blocks, _, conv, frames, padding = rsup.plan(lib, rs, n)
        cur, got = asup.cursor(lib), []
        for at in range(0, n, FS):
            got += asup.plan_call(lib, rs, cur, min(FS, n - at))
        tail, pad = asup.plan_flush(lib, rs, cur)
        assert keys(got + tail) == keys(blocks), "n = %d" % n
        assert (cur.fed, cur.frames, pad) == (conv, frames, padding), "n = %d" % n


def first_tap(rs, start, k):
    """lh_rs_locate's `first' (csrc/lh_rs_sample.h): every step a double operation, as there"""
    return math.floor(k * rs.ratio - start) - rs.taps // 2


def span(rs, t):
    return first_tap(rs, t.start, t.k0 + t.count - 1) + rs.taps + 1 - first_tap(rs, t.start, t.k0)


def all_blocks(lib, rs, pattern):
    cur, blocks = asup.cursor(lib), []
    for m in pattern:
        blocks += asup.plan_call(lib, rs, cur, m)
    return blocks + asup.plan_flush(lib, rs, cur)[0]


@pytest.mark.parametrize("rate_in,rate_out", PAIRS, ids=PAIR_IDS)
def test_tiles_partition_their_block_within_the_span(rate_in, rate_out, lib):
    """the tiles of every block cover its outputs in order, each touches at most LH_RS_SPAN_MAX input positions and is as
    large as fits; a block that makes nothing has none.  96 -> 32 kHz fed 9000 samples at once really is cut (a block of
    1152 outputs spans about 3490 positions: three tiles or more), 44.1 -> 48 kHz never is (a block spans less input than
    it makes output)"""
    rs = rsup.resampler(lib, rate_in, rate_out)
    most = 0
    for pattern in patterns(rate_in) + [[9000]]:
        for b in all_blocks(lib, rs, pattern):
            tiles = asup.block_tiles(lib, rs, b, stream=5)
            assert (len(tiles) > 0) == (b.made > 0)
            k = 0
            for j, t in enumerate(tiles):
                assert (t.k0, t.out_at, t.in_at, t.start, t.stream) == (k, b.out_at + k, b.in_at, b.start, 5)
                assert t.count >= 1 and span(rs, t) <= asup.SPAN_MAX
                if j + 1 < len(tiles):
                    more = asup.LhRsTile.from_buffer_copy(t)
                    more.count += 1
                    assert span(rs, more) > asup.SPAN_MAX
                k += t.count
            assert k == b.made
            if pattern == [9000]:
                most = max(most, len(tiles))
            if (rate_in, rate_out) == (44100, 48000):
                assert len(tiles) <= 1
    if (rate_in, rate_out) == (96000, 32000):
        assert most >= 3


EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_resample")


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make([], EMU_DIR)
    e = C.CDLL(os.path.join(EMU_DIR, "libhipemu_resample.so"))
    e.lh_emu_resample_tiles.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    return e


# (sample type, (name, channels, pcm_scale, pcm_mix, pcm_scale_r, one plane)): the four matrices of tests/test_pcm_input.py
EMU_CASES = [(PCM_S16, tai.MATRICES[0]), (PCM_S32, tai.MATRICES[1]), (PCM_F32_UNIT, tai.MATRICES[2]), (PCM_F32_UNIT, tai.MATRICES[3]),
             (PCM_S16, tai.MATRICES[3])]
# what the three streams get in round 1 and round 2 (a stream with nothing in a round, empty calls, one large call)
ROUNDS = [[[4000, 1, 1153], [], [9000, 0, 33]], [[575, 6271], [3, 1152, 10845], [2967]]]


@pytest.mark.parametrize("case", range(len(EMU_CASES)), ids=["%s-%s" % (psup.TYPE_NAMES[t], m[0]) for t, m in EMU_CASES])
@pytest.mark.parametrize("rate_in,rate_out", PAIRS, ids=PAIR_IDS)
def test_tile_kernel_source_matches_the_host_chain(rate_in, rate_out, case, lib, emu):
    """csrc/lh_resample_dev.hip: lh_resample_tiles_kernel under the fiber emulator -- three streams of 12 000 input samples
    fed in two ragged rounds and the finish, one launch per round over the tiles planned for it, the stream lengths of
    that round in the launch's table.  The input pool holds NaN (0x7fff) beyond what each stream has been fed so far, the
    right row of a one-plane batch all over, and the float pool a NaN pattern before the first round: after every round
    the float pool is the host chain (lh_rs_block call by call; at the end the flush) float for float in
    [0, converted) and the NaN pattern everywhere else, and a round's table in reversed order gives the same pool."""
    stype, (_, channels, scale, mix, scale_r, one_plane) = EMU_CASES[case]
    plib = psup.library()
    dtype = lamehip.PCM_DTYPES[stype]
    m = psup.matrix(plib, stype, scale, mix, scale_r)
    rs = rsup.resampler(lib, rate_in, rate_out)
    B = 3
    assert all(sum(ROUNDS[0][s]) + sum(ROUNDS[1][s]) == 12000 for s in range(B))
    xs = [psup.typed_signal(stype, 5300 + 10 * case + s, 12000, rate_in) for s in range(B)]
    behind = [psup.host_ingest(plib, stype, m, x[0], None if one_plane else x[1]) for x in xs]
    cap_in, cap_out = 12000 + 5, int(12000 * rate_out / rate_in) + 4 * FS + 64
    beyond = psup.beyond_value(stype)
    pool = np.full((B, 2, cap_in), beyond, dtype)
    marker = np.frombuffer(np.uint32(0x7fc00abc).tobytes(), np.float32)[0]
    pools = [np.full((B, 2, cap_out), marker, np.float32) for _ in range(2)]
    bank = np.zeros((2 * rs.phases + 1, rsup.LH_RS_ROW), np.float32)
    bank[:, :34] = np.ctypeslib.as_array(rs.bank)[:2 * rs.phases + 1]
    bank[:, rs.taps + 1:] = 0
    p = rsup.LhRsParams()
    p.ratio, p.taps, p.phases, p.channels = rs.ratio, rs.taps, rs.phases, channels
    p.m = rsup.LhRsMatrix(*[float(v) for v in m])
    p.one_plane, p.cap_in, p.cap_out = int(one_plane), cap_in, cap_out
    chains = [asup.HostChain(lib, rate_in, rate_out, channels) for _ in range(B)]
    curs = [asup.cursor(lib) for _ in range(B)]
    fed = [0] * B
    for rnd in range(3):
        tiles = []
        for s in range(B):
            if rnd < 2:
                for n in ROUNDS[rnd][s]:
                    pool[s, 0, fed[s]:fed[s] + n] = xs[s][0, fed[s]:fed[s] + n]
                    if not one_plane:
                        pool[s, 1, fed[s]:fed[s] + n] = xs[s][1, fed[s]:fed[s] + n]
                    chains[s].call(behind[s][:, fed[s]:fed[s] + n])
                    blocks = asup.plan_call(lib, rs, curs[s], n)
                    fed[s] += n
                    for b in blocks:
                        tiles += asup.block_tiles(lib, rs, b, s)
            else:
                chains[s].flush()
                for b in asup.plan_flush(lib, rs, curs[s])[0]:
                    tiles += asup.block_tiles(lib, rs, b, s)
        assert tiles or rnd < 2
        lens = (C.c_longlong * B)(*fed)
        for out, order in zip(pools, (tiles, tiles[::-1])):
            arr = (asup.LhRsTile * max(len(order), 1))(*order)
            assert emu.lh_emu_resample_tiles(stype, C.byref(p), bank.ctypes.data, arr, len(order), lens, pool.ctypes.data,
                                             out.ctypes.data) == 0
        for s in range(B):
            want = chains[s].floats()
            k = want.shape[1]
            assert k == curs[s].fed
            assert rsup.same_floats(pools[0][s, :, :k], want), "round %d stream %d" % (rnd, s)
            assert pools[0][s, :, k:].tobytes() == np.full((2, cap_out - k), marker, np.float32).tobytes(), \
                "round %d stream %d: written beyond its converted length" % (rnd, s)
            if channels == 1:
                assert not want[1].any()
        assert pools[0].tobytes() == pools[1].tobytes(), "round %d: the order of the table shows" % rnd
    assert max(t.count for t in tiles) > 0 and all(curs[s].frames > 0 for s in range(B))


@pytest.fixture(scope="module")
def emu_ingest():
    d = os.path.join(helpers.ROOT, "tests", "hipemu_ingest")
    helpers.locked_make([], d)
    e = C.CDLL(os.path.join(d, "libhipemu_ingest.so"))
    e.lh_emu_append_raw.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
    return e


RAW_LENGTHS = [0, 1, 3, 4, 5, 4099]


@pytest.mark.parametrize("one_plane", [False, True], ids=["two-planes", "one-plane"])
def test_as_it_is_append_keeps_every_bit(one_plane, emu_ingest):
    """csrc/lh_ingest.hip: lh_append_kernel for 4-byte elements as they are (the input pool of a typed batch that converts
    round by round) under the emulator: every residue of `at' mod 4, stride 1 and 2, lengths 0 .. 4099, sources at all
    four offsets from a 16-byte boundary.  The samples are bit patterns no arithmetic would leave alone -- NaNs with
    payloads (quiet and signalling), -0.0, infinities, denormals, random words --: the pool holds exactly them inside
    every [at, at + n) and its marker everywhere else; with one plane the right source (all poison) is never read and the
    right row mirrors the left.  A matrix in the parameters changes nothing."""
    rng = np.random.default_rng(6100 + int(one_plane))
    cap, marker, special = 4200, 0xa5a5a5a5, [0x7fc12345, 0xffc00001, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000, 1, 0x807fffff]
    table = []                      # (stream, at, n, stride, offset of the left source, of the right source)
    for i, n in enumerate(RAW_LENGTHS):
        for res in range(4):
            j = 4 * i + res
            table.append((j, 8 + res + 4 * (j % 3), n, 1 + (i + res) % 2, 4 * ((res + i) % 4), 4 * ((res + 2 * i + 1) % 4)))
    assert {(t[1] % 4, t[3]) for t in table} == {(r, st) for r in range(4) for st in (1, 2)}
    assert all(t[1] + t[2] <= cap for t in table)
    nstreams = len(table) + 1       # (the last one has no segment)
    segs, wants, keep = [], [], []
    for s, at, n, stride, off_l, off_r in table:
        x = rng.integers(0, 1 << 32, (2, n), dtype=np.uint64).astype(np.uint32)
        x[:, :len(special)] = np.array(special, np.uint32)[:n]
        xf = x.view(np.float32)
        pl, pr, held = tai.source(PCM_F32_UNIT, xf, stride, one_plane, off_l, off_r)
        keep.append(held)
        segs.append(tai.LhApSeg(pl, pr, at, n, s, stride))
        wants.append(np.stack([x[0], x[0] if one_plane else x[1]]))
    p = psup.LhInParams()
    p.m[:] = [0.5, 0.25, 0.0, 3.0]
    p.channels, p.one_plane, p.cap = 2 - int(one_plane), int(one_plane), cap
    pool = tai.aligned_pool((nstreams, 2, cap), np.uint32, marker)
    arr = (tai.LhApSeg * len(segs))(*segs)
    assert emu_ingest.lh_emu_append_raw(4, C.byref(p), arr, len(segs), max(RAW_LENGTHS), pool.ctypes.data) == 0
    untouched = np.ones(pool.shape, bool)
    for j, (s, at, n, _, _, _) in enumerate(table):
        assert pool[s, :, at:at + n].tobytes() == wants[j].tobytes(), "segment %d" % j
        untouched[s, :, at:at + n] = False
    assert (pool[untouched] == marker).all(), "written outside the segments"


def test_plan_functions_under_sanitizers():
    """tests/rs_plan_check: lh_rs_plan_call, lh_rs_plan_flush and lh_rs_block_tiles as a program of its own over the rate
    pairs and seeded call patterns above, built with AddressSanitizer and UBSan (host code only, no GPU)"""
    d = os.path.join(helpers.ROOT, "tests", "rs_plan_check")
    helpers.locked_make(["rs_plan_check"], d)
    r = subprocess.run([os.path.join(d, "rs_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:]
    assert r.stdout.count(" Hz, ") == 3 * len(PAIRS)


def test_switch_is_declared_and_exported():
    lib = lamehip.load_library()
    txt = open(os.path.join(helpers.ROOT, "include", "lamehip.h")).read()
    assert "lamehip_batch_set_incremental_resampling(" in txt and hasattr(lib, "lamehip_batch_set_incremental_resampling")
