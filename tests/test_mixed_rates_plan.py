"""Incremental converting batches whose streams arrive at rates of their own (lamehip_batch_set_stream_in_samplerate), the
parts that need no GPU: the pass-through plan of a stream the reference does not convert (csrc/lh_resample.c:
lh_rs_init_identity behind lh_rs_plan_call / _flush), the tiles' class, the SOURCE of the mixed kernel
(csrc/lh_resample_dev.hip: lh_resample_mixed_tiles_kernel) under the fiber emulator of tests/hipemu over one ragged round
table of nine streams at nine rates, and the tag frame's info byte of a stream at its own rate.  Floats and bytes are
compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import append_resample_support as asup
import helpers
import lamehip
import mixed_rates_support as msup
import pcm_input_support as psup
import resample_support as rsup
import test_append_input as tai
from lamehip import PCM_F32_UNIT, PCM_S16
from mixed_rates_support import OUT, RATES
from resample_support import FS

EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_rs_mixed")


@pytest.fixture(scope="module")
def lib():
    return msup.library()


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_rs_mixed.so"], EMU_DIR)
    e = C.CDLL(os.path.join(EMU_DIR, "libhipemu_rs_mixed.so"))
    e.lh_emu_resample_mixed_tiles.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    e.lh_emu_resample_tiles.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    return e


def test_taps_phases_and_the_bypass_window(lib):
    """what lh_rs_init resolves for the pool's rates, and which of them the reference passes through: 44077 .. 44122 Hz for
    44.1 kHz out (reference util.c:656-657)"""
    want = {48000: (31, 147), 32000: (31, 320), 22050: (31, 2), 88200: (32, 1), 96000: (31, 147), 8000: (31, 320),
            44130: (31, 320)}
    for hz in RATES:
        rs = msup.converter(lib, hz)
        if hz in want:
            assert lib.lh_rs_needed(hz, OUT) == 1 and not lib.lh_rs_is_identity(C.byref(rs))
            assert (rs.taps, rs.phases) == want[hz], hz
            assert rs.ratio == hz / OUT
        else:
            assert lib.lh_rs_needed(hz, OUT) == 0 and lib.lh_rs_is_identity(C.byref(rs))
            assert (rs.taps, rs.phases, rs.ratio, rs.rate_in) == (0, 0, 1.0, hz)
    assert [hz for hz in range(44060, 44140) if not lib.lh_rs_needed(hz, OUT)] == list(range(44077, 44123))
    assert 44077 == int(np.float32(OUT) * np.float32(0.9995)) and 44122 == int(np.float32(OUT) * np.float32(1.0005))


def noise(seed, n):
    return (np.random.default_rng(seed).standard_normal((2, n)) * 9000).astype(np.float32)


@pytest.mark.parametrize("hz", [44100, 44110])
def test_pass_through_plan_is_fill_buffers(hz, lib):
    """a stream that is not converted: after every call the plan's blocks and cursor are fill_buffer's -- made = used =
    min(frame, what is left of the call), no clock --, and the flush is lame_encode_flush's without a converter's delay:
    blocks, converted length, frames, mf_size and padding.  Where the reference is built, frames and padding are its own
    for the same calls (the frame count by its bytes' headers, the padding from its tag frame)."""
    rs = msup.converter(lib, hz)
    rng = np.random.default_rng(hz)
    patterns = [msup.CHUNKS, [4000, 0, 1153, 1, 1152, 1151], [int(v) for v in rng.choice([0, 1, 575, 1152, 1153, 4000, 9000], 12)]]
    for pi, pattern in enumerate(patterns):
        chain, cur = msup.PassChain(1), asup.cursor(lib)
        for ci, m in enumerate(pattern):
            want = chain.call(noise(ci, m))
            got = asup.plan_call(lib, rs, cur, m)
            assert [b.key() for b in got] == want, (pi, ci)
            assert asup.cursor_key(cur) == chain.state()
            assert all(b.made == min(FS, b.len) for b in got)
        want, want_padding = chain.flush()
        got, padding = asup.plan_flush(lib, rs, cur)
        assert [b.key() for b in got] == want and padding == want_padding
        assert asup.cursor_key(cur) == chain.state() and cur.nblk == len(chain.blocks)
        n = sum(pattern)
        # (what the one-shot path knows of a stream of n samples that is not converted)
        assert cur.frames == lib.lh_total_frames_fs(C.c_long(n), FS) and padding == lib.lh_end_padding_fs(C.c_long(n), FS)
        if helpers.have_reference():
            frames, pad = reference_frames_and_padding(hz, pattern)
            assert (cur.frames, padding) == (frames, pad), (hz, pi)
        # every block is one tile, with the class written into it
        for b in got:
            tiles = msup.block_tiles(lib, rs, b, 3, 7)
            assert len(tiles) == (1 if b.made else 0)
            for t in tiles:
                assert (t.k0, t.count, t.in_at, t.out_at, t.stream, t.pad_) == (0, b.made, b.in_at, b.out_at, 3, 7)


def reference_frames_and_padding(hz, pattern):
    """the compiled reference at (in = hz, out = 44.1 kHz, tag on) fed the pattern's calls: frames encoded (without the
    placeholder) and the end padding in its tag frame"""
    ref = helpers.Reference()
    lib = ref.lib
    lib.refh_option.argtypes = [C.c_char_p, C.c_float]
    lib.refh_open_tag.restype = C.c_void_p
    lib.refh_option(None, 0)
    lib.refh_option(b"out_samplerate", float(OUT))
    try:
        h = C.c_void_p(lib.refh_open_tag(hz, 128, -1, -1))
    finally:
        lib.refh_option(None, 0)
    assert h
    buf = C.create_string_buffer(200000)
    x = helpers.synth_stream(hz, max(sum(pattern), 1), 44100)
    at = 0
    for m in pattern:
        l, r = np.ascontiguousarray(x[0, at:at + m]), np.ascontiguousarray(x[1, at:at + m])
        assert lib.refh_encode(h, l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), m, buf, len(buf)) >= 0
        at += m
    assert lib.refh_flush(h, buf, len(buf)) >= 0
    frames = lib.refh_frame_number(h)
    t = C.create_string_buffer(2880)
    k = lib.refh_lametag(h, t, len(t))
    lib.refh_close(h)
    tag = t.raw[:k]
    at = tag.index(b"Info") + 116 + 25
    return frames, ((tag[at + 1] & 0x0f) << 8) | tag[at + 2]


@pytest.mark.parametrize("hz", [48000, 96000, 8000])
def test_tiles_carry_their_class(hz, lib):
    """lh_rs_block_tiles_class cuts what lh_rs_block_tiles cuts and writes the class; lh_rs_block_tiles writes class 0"""
    rs = msup.converter(lib, hz)
    cur = asup.cursor(lib)
    for b in asup.plan_call(lib, rs, cur, 4000) + asup.plan_flush(lib, rs, cur)[0]:
        plain, classed = asup.block_tiles(lib, rs, b, 2), msup.block_tiles(lib, rs, b, 2, 9)
        assert [(t.k0, t.count, t.in_at, t.out_at, t.start, t.stream) for t in plain] == \
            [(t.k0, t.count, t.in_at, t.out_at, t.start, t.stream) for t in classed]
        assert all(t.pad_ == 0 for t in plain) and all(t.pad_ == 9 for t in classed)


# (sample type, (name, channels, pcm_scale, pcm_mix, pcm_scale_r, one plane)): stereo and mono, s16 and float32 at +-1.0
EMU_CASES = [(PCM_S16, tai.MATRICES[0]), (PCM_F32_UNIT, tai.MATRICES[1]), (PCM_S16, tai.MATRICES[3]), (PCM_F32_UNIT, tai.MATRICES[2])]


def class_table(lib, rates):
    """converters, class records and the banks' one allocation for `rates' (class c = rates[c])"""
    convs = [msup.converter(lib, hz) for hz in rates]
    recs = (msup.LhRsClass * len(rates))()
    banks = np.zeros((len(rates), msup.BANK_FLOATS), np.float32)
    for c, rs in enumerate(convs):
        recs[c].ratio, recs[c].taps, recs[c].phases = rs.ratio, rs.taps, rs.phases
        recs[c].identity = int(bool(lib.lh_rs_is_identity(C.byref(rs))))
        recs[c].bank_at = c * msup.BANK_FLOATS
        if not recs[c].identity:
            rows = banks[c].reshape(641, rsup.LH_RS_ROW)
            rows[:2 * rs.phases + 1, :rs.taps + 1] = np.ctypeslib.as_array(rs.bank)[:2 * rs.phases + 1, :rs.taps + 1]
        else:
            banks[c] = np.nan           # (a class that is not converted reads no bank)
    return convs, recs, banks


@pytest.mark.parametrize("case", range(len(EMU_CASES)), ids=["%s-%s" % (psup.TYPE_NAMES[t], m[0]) for t, m in EMU_CASES])
def test_mixed_kernel_source_matches_the_host_chains(case, lib, emu):
    """csrc/lh_resample_dev.hip: lh_resample_mixed_tiles_kernel under the fiber emulator -- nine streams at nine rates, all to
    44.1 kHz, fed in six ragged rounds (0, 1, 1151, 1152, 1153 and 4000 samples, rotated: every round has a stream, hence
    a class, without a tile, and neighbouring tiles of different classes), one more round and the flush, ONE launch per
    round over all classes' tiles.  The input pool holds NaN (0x7fff) beyond what each stream has been fed, the float pool a
    NaN pattern: after every round every stream's floats are its host chain's at its own rate -- lh_rs_block call by call,
    fill_buffer's copy for the two rates the reference passes through -- float for float in [0, converted) and the
    pattern everywhere else, and the round's table in reversed order gives the same pool.  96 kHz blocks really are cut
    into several tiles.  A tile whose class is out of range, and one whose outputs leave the row, write nothing."""
    stype, (_, channels, scale, mix, scale_r, one_plane) = EMU_CASES[case]
    plib = psup.library()
    dtype = lamehip.PCM_DTYPES[stype]
    m = psup.matrix(plib, stype, scale, mix, scale_r)
    B = len(RATES)
    convs, recs, banks = class_table(lib, RATES)
    rounds = msup.rounds_of(B, extra=2600)
    total = [sum(r[s] for r in rounds) for s in range(B)]
    xs = [psup.typed_signal(stype, 6300 + 10 * case + s, total[s], RATES[s]) for s in range(B)]
    behind = [psup.host_ingest(plib, stype, m, x[0], None if one_plane else x[1]) for x in xs]
    cap_in = max(total) + 3
    cap_out = max(int(total[s] * OUT / RATES[s]) for s in range(B)) + 4 * FS + 64
    pool = np.full((B, 2, cap_in), psup.beyond_value(stype), dtype)
    marker = np.frombuffer(np.uint32(0x7fc00abc).tobytes(), np.float32)[0]
    pools = [np.full((B, 2, cap_out), marker, np.float32) for _ in range(2)]
    p = rsup.LhRsParams()
    p.ratio, p.taps, p.phases, p.channels = 0.0, 0, 0, channels           # (the mixed kernel looks at its classes)
    p.m = rsup.LhRsMatrix(*[float(v) for v in m])
    p.one_plane, p.cap_in, p.cap_out = int(one_plane), cap_in, cap_out
    chains = [msup.chain(lib, hz, channels) for hz in RATES]
    curs = [asup.cursor(lib) for _ in range(B)]
    fed = [0] * B
    most_tiles = {}
    for rnd in range(len(rounds) + 1):
        tiles = []
        for s in range(B):
            if rnd < len(rounds):
                n = rounds[rnd][s]
                pool[s, 0, fed[s]:fed[s] + n] = xs[s][0, fed[s]:fed[s] + n]
                if not one_plane:
                    pool[s, 1, fed[s]:fed[s] + n] = xs[s][1, fed[s]:fed[s] + n]
                chains[s].call(behind[s][:, fed[s]:fed[s] + n])
                blocks = asup.plan_call(lib, convs[s], curs[s], n)
                fed[s] += n
            else:
                chains[s].flush()
                blocks = asup.plan_flush(lib, convs[s], curs[s])[0]
            for b in blocks:
                cut = msup.block_tiles(lib, convs[s], b, s, s)
                most_tiles[s] = max(most_tiles.get(s, 0), len(cut))
                tiles += cut
        if rnd < len(msup.CHUNKS):
            assert {t.stream for t in tiles} != set(range(B)), "every class has a tile in round %d" % rnd
        assert any(a.pad_ != b.pad_ for a, b in zip(tiles, tiles[1:]))
        # two tiles the kernel has to leave alone: no such class; outputs that leave the row
        stray = [asup.LhRsTile.from_buffer_copy(tiles[0]), asup.LhRsTile.from_buffer_copy(tiles[0])]
        stray[0].pad_ = B
        stray[1].out_at = cap_out - stray[1].count + 1
        lens = (C.c_longlong * B)(*fed)
        for out, order in zip(pools, (tiles + stray, stray + tiles[::-1])):
            arr = (asup.LhRsTile * len(order))(*order)
            assert emu.lh_emu_resample_mixed_tiles(stype, C.byref(p), recs, B, banks.ctypes.data, arr, len(order), lens,
                                                   pool.ctypes.data, out.ctypes.data) == 0
        for s in range(B):
            want = chains[s].floats()
            k = want.shape[1]
            assert k == curs[s].fed
            assert rsup.same_floats(pools[0][s, :, :k], want), "round %d stream %d (%d Hz)" % (rnd, s, RATES[s])
            assert pools[0][s, :, k:].tobytes() == np.full((2, cap_out - k), marker, np.float32).tobytes(), \
                "round %d stream %d: written beyond its converted length" % (rnd, s)
            if channels == 1:
                assert not want[1].any()
        assert pools[0].tobytes() == pools[1].tobytes(), "round %d: the order of the table shows" % rnd
    assert most_tiles[RATES.index(96000)] >= 2 and most_tiles[RATES.index(44100)] == 1
    assert all(curs[s].frames > 0 for s in range(B))


def test_class_zero_tiles_are_the_single_rate_kernels(lib, emu):
    """a round of one class through the mixed kernel gives the floats lh_resample_tiles_kernel gives: one text"""
    hz, n = 48000, 5000
    convs, recs, banks = class_table(lib, [hz])
    rs = convs[0]
    x = psup.typed_signal(PCM_S16, 77, n, hz)
    pool = np.zeros((1, 2, n), np.int16)
    pool[0] = x
    cur, tiles = asup.cursor(lib), []
    for b in asup.plan_call(lib, rs, cur, n) + asup.plan_flush(lib, rs, cur)[0]:
        tiles += msup.block_tiles(lib, rs, b, 0, 0)
    cap_out = int(cur.fed) + 5
    p = rsup.LhRsParams()
    p.ratio, p.taps, p.phases, p.channels = rs.ratio, rs.taps, rs.phases, 2
    p.m = rsup.LhRsMatrix(1.0, 0.0, 0.0, 1.0)
    p.one_plane, p.cap_in, p.cap_out = 0, n, cap_out
    outs = [np.zeros((1, 2, cap_out), np.float32) for _ in range(2)]
    arr = (asup.LhRsTile * len(tiles))(*tiles)
    lens = (C.c_longlong * 1)(n)
    assert emu.lh_emu_resample_mixed_tiles(PCM_S16, C.byref(p), recs, 1, banks.ctypes.data, arr, len(tiles), lens,
                                           pool.ctypes.data, outs[0].ctypes.data) == 0
    bank = np.ascontiguousarray(banks[0].reshape(641, rsup.LH_RS_ROW)[:2 * rs.phases + 1])
    assert emu.lh_emu_resample_tiles(PCM_S16, C.byref(p), bank.ctypes.data, arr, len(tiles), lens, pool.ctypes.data,
                                     outs[1].ctypes.data) == 0
    assert outs[0].tobytes() == outs[1].tobytes() and outs[0][0, :, :cur.fed].any()


def reference_info_byte(hz):
    """the info byte of the reference's lame_get_lametag_frame at (in = hz, out = 44.1 kHz), CBR 128"""
    ref = helpers.Reference()
    ref.lib.refh_option.argtypes = [C.c_char_p, C.c_float]
    ref.lib.refh_option(None, 0)
    ref.lib.refh_option(b"out_samplerate", float(OUT))
    try:
        _, tag = helpers.reference_tagged(helpers.synth_stream(5, hz // 5, 44100), hz, 128)
    finally:
        ref.lib.refh_option(None, 0)
    return tag[tag.index(b"Info") + 116 + 28]


def test_tag_info_byte_under_sanitizers():
    """tests/hipemu_rs_mixed/tag_info_host_check (its own main; AddressSanitizer and UBSan linked in): the batch's template
    with the stream's info byte out of the padding table's entry, finished, is lh_tag_frame at the stream's rate -- the byte
    and both CRCs -- for batches at four rates, CBR and VBR, with and without the header CRC.  Where the reference is built,
    the byte at 8000, 32000, 44100, 48000 and 96000 Hz in is that of its lame_get_lametag_frame."""
    helpers.locked_make(["tag_info_host_check"], EMU_DIR)
    r = subprocess.run([os.path.join(EMU_DIR, "tag_info_host_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "FAILED" not in r.stdout, r.stdout[-2000:]
    info = {int(l.split()[1]): int(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("rate ")}
    assert {8000, 32000, 44100, 48000, 96000} <= set(info)
    if helpers.have_reference():
        for hz in (8000, 32000, 44100, 48000, 96000):
            assert info[hz] == reference_info_byte(hz), hz


def test_calls_are_declared_exported_and_bound():
    lib = lamehip.load_library()
    txt = open(os.path.join(helpers.ROOT, "include", "lamehip.h")).read()
    for name in ("lamehip_batch_set_stream_in_samplerate", "lamehip_batch_stream_in_samplerate"):
        assert name + "(" in txt and hasattr(lib, name), name
    for name in ("lh_launch_resample_mixed_tiles", "lh_rs_init_identity", "lh_rs_block_tiles_class"):
        assert hasattr(lib, name), name
    for name in ("set_stream_in_samplerate", "stream_in_samplerate"):
        assert hasattr(lamehip.Batch, name), name
