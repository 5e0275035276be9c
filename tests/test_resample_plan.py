"""The batch's rate conversion as a plan (csrc/lh_resample.c: lh_rs_plan, lh_rs_trunk_extend, lh_rs_plan_tail): which
blocks there are follows from the rates and the stream's length alone, and given its block an output sample depends on
nothing but the stream's input (csrc/lh_rs_sample.h).  Checked against lh_rs_block driven the way a batch's host
conversion drives it, against the oracle's restatement of the converter, and -- the device kernel's SOURCE run by the
fiber emulator of tests/hipemu -- against the host conversion."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import resample_support as rsup
from resample_support import FS, MFN, MF_START

PAIRS = [(44100, 32000), (48000, 44100), (22050, 44100), (44100, 48000), (96000, 48000), (37800, 44100), (8000, 32000),
         (48000, 32000), (11025, 32000)]          # the last one: more phases than the bank's cap of 320


def lengths(rate_in):
    return [0, 1, 16, 1151, 1152, 1153, 2304, 5000, rate_in // 2 + 13]


# (channels, pcm_scale, pcm_mix, pcm_scale_r): both channels behind a mixing matrix with different scales, mono
# without a downmix (the second plane mirrors the first), mono as a downmix
MATRICES = [(2, 0.8, 0.3, 0.6), (1, 0.9, 0.0, 0.9), (1, 0.5, 0.5, 0.5)]


@pytest.fixture(scope="module")
def lib():
    return rsup.library()


def signal(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((2, n)) * 9000).clip(-32768, 32767).astype(np.int16)


def drive_blocks(lib, rate_in, rate_out, x):
    """lh_rs_block on channel 0 of the float signal x, called as the batch's host conversion calls it (a frame of input
    per call, then the flush): the blocks as (in_at, out_at, start, len, made), converted length, frames, padding"""
    rs = rsup.resampler(lib, rate_in, rate_out)
    ratio = rs.ratio
    blocks, out = [], np.zeros(FS, np.float32)
    state = dict(fed=0, mf=MF_START, frames=0, at=0)

    def feed(src, m):
        pos = 0
        while m > 0:
            used = C.c_int(0)
            start = rs.clock[0]
            buf = np.ascontiguousarray(src[pos:pos + m])
            made = lib.lh_rs_block(C.byref(rs), 0, out.ctypes.data, FS, buf.ctypes.data, m, C.byref(used))
            blocks.append((state["at"], state["fed"], start, m, made))
            state["fed"] += made
            state["mf"] += made
            if state["mf"] >= MFN:
                state["frames"] += 1
                state["mf"] -= FS
            assert used.value > 0
            state["at"] += used.value
            pos += used.value
            m -= used.value

    for p in range(0, len(x), FS):
        feed(x[p:p + FS], min(FS, len(x) - p))
    owed = int(576 + state["fed"] - FS * state["frames"])
    owed = int(owed + 16. / ratio)
    padding = FS - owed % FS
    if padding < 576:
        padding += FS
    left = (owed + padding) // FS
    zeros = np.zeros(1152, np.float32)
    while left > 0:
        before = state["frames"]
        bunch = max(1, min(1152, int((MFN - state["mf"]) * ratio)))
        feed(zeros, bunch)
        left -= 1 if state["frames"] != before else 0
    return blocks, state["fed"], state["frames"], padding


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_plan_equals_block_by_block_conversion(rate_in, rate_out, lib):
    """blocks, converted length, frames and padding of the plan are those of lh_rs_block / the host conversion, and the
    plan evaluated sample by sample gives the host conversion's floats bit for bit"""
    rs = rsup.resampler(lib, rate_in, rate_out)
    for n in lengths(rate_in):
        pcm = signal(rate_in + n, n)
        blocks, ntrunk, conv, frames, padding = rsup.plan(lib, rs, n)
        want_blocks, want_conv, want_frames, want_padding = drive_blocks(lib, rate_in, rate_out, pcm[0].astype(np.float32))
        assert [b.key() for b in blocks] == want_blocks, "n = %d" % n
        assert (conv, frames, padding) == (want_conv, want_frames, want_padding), "n = %d" % n
        assert 0 <= ntrunk <= len(blocks)
        for channels, scale, mix, scale_r in MATRICES:
            want, hframes, hpadding = rsup.host_convert(lib, rate_in, rate_out, channels, scale, mix, scale_r, pcm)
            assert (want.shape[1], hframes, hpadding) == (conv, frames, padding), "n = %d" % n
            got = rsup.evaluate(lib, rs, blocks, conv, channels, scale, mix, scale_r, pcm)
            assert rsup.same_floats(got, want), "n = %d, matrix %r" % (n, (channels, scale, mix, scale_r))
            if channels == 1:
                assert not want[1].any()


@pytest.mark.parametrize("case", [1, 3, 9])
def test_plan_equals_oracle_restatement(case, lib, oracle):
    """the floats of the evaluated plan are the oracle's (orc_resample_stream, call pattern [1152]), which the existing
    tests pin to the reference"""
    import test_resample
    rate_in, kw, out, rate_out = test_resample.CASES[case]
    enc = test_resample.open_product(rate_in, kw, out, require_device=False)
    cfg = enc.config()
    enc.close()
    assert cfg.samplerate == rate_out
    n = rate_in // 2 + 13
    pcm = helpers.synth_stream(7400 + case, n, rate_in, 1.0 / 9)
    cap = int(n * rate_out / rate_in) + 8192
    fl, fr = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    nf, pad = C.c_int(0), C.c_int(0)
    pat = (C.c_int * 1)(1152)
    olib = oracle.lib
    olib.orc_resample_stream.restype = C.c_long
    k = olib.orc_resample_stream(C.byref(cfg), rate_in, pcm[0].ctypes.data_as(C.c_void_p),
                                 np.ascontiguousarray(pcm[1]).ctypes.data_as(C.c_void_p), C.c_long(n), pat, 1,
                                 fl.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p), C.c_long(cap), C.byref(nf),
                                 C.byref(pad))
    assert 0 < k <= cap
    rs = rsup.resampler(lib, rate_in, rate_out)
    blocks, ntrunk, conv, frames, padding = rsup.plan(lib, rs, n)
    assert (conv, frames, padding) == (k, nf.value, pad.value)
    got = rsup.evaluate(lib, rs, blocks, conv, cfg.channels, cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r, pcm)
    assert rsup.same_floats(got, np.stack([fl[:k], fr[:k]]))


@pytest.mark.parametrize("rate_in,rate_out", [(48000, 44100), (8000, 32000), (96000, 48000)])
def test_plan_is_shared_trunk_plus_own_tail(rate_in, rate_out, lib):
    """the blocks of a stream's full chunks are those of every longer stream"""
    rs = rsup.resampler(lib, rate_in, rate_out)
    long_blocks, long_trunk, _, _, _ = rsup.plan(lib, rs, 20 * FS + 77)
    assert long_trunk > 0
    for n in (0, 5, FS, FS + 1, 7 * FS - 1, 7 * FS, 19 * FS + 500, 20 * FS):
        blocks, ntrunk, _, _, _ = rsup.plan(lib, rs, n)
        assert ntrunk <= long_trunk
        assert [b.key() for b in blocks[:ntrunk]] == [b.key() for b in long_blocks[:ntrunk]]
        # the prefix is the full chunks, no more and no less
        assert all(b.in_at + b.len <= n // FS * FS for b in blocks[:ntrunk])
        assert all(b.in_at >= n // FS * FS for b in blocks[ntrunk:])
        assert len(blocks) > ntrunk          # (the flush is always the stream's own)


EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_resample")


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make([], EMU_DIR)
    return C.CDLL(os.path.join(EMU_DIR, "libhipemu_resample.so"))


@pytest.mark.parametrize("rate_in,rate_out,matrix", [(48000, 44100, MATRICES[0]), (22050, 44100, MATRICES[1]),
                                                     (11025, 32000, MATRICES[2])])
def test_kernel_source_matches_host_conversion(rate_in, rate_out, matrix, lib, emu):
    """csrc/lh_resample_dev.hip under the fiber emulator: four ragged streams over one shared trunk, rows filled with
    0x7fff beyond each stream's length (they must not be read), against the host conversion bit for bit"""
    channels, scale, mix, scale_r = matrix
    lens = [3 * FS + 401, 0, 2 * FS, 700]
    cap_in = max(lens) + 64
    rs = rsup.resampler(lib, rate_in, rate_out)
    trunk = rsup.LhRsTrunk()
    lib.lh_rs_trunk_init(C.byref(trunk), FS, MFN)
    assert lib.lh_rs_trunk_extend(C.byref(rs), C.byref(trunk), max(lens) // FS) == 0
    pcms = [signal(900 + s, n) for s, n in enumerate(lens)]
    wants = [rsup.host_convert(lib, rate_in, rate_out, channels, scale, mix, scale_r, x)[0] for x in pcms]
    cap_out = max(w.shape[1] for w in wants) + 64
    tails, streams, max_blocks = [], (rsup.LhRsStream * len(lens))(), 0
    for s, n in enumerate(lens):
        tail = (rsup.LhRsBlock * 64)()
        conv, frames, padding = C.c_long(0), C.c_int(0), C.c_int(0)
        k = lib.lh_rs_plan_tail(C.byref(rs), C.byref(trunk), n, tail, 64, C.byref(conv), C.byref(frames), C.byref(padding))
        assert 0 < k <= 64 and conv.value == wants[s].shape[1]
        streams[s] = rsup.LhRsStream(n, s, trunk.after[n // FS].nblk, len(tails), k)
        tails += list(tail[:k])
        max_blocks = max(max_blocks, streams[s].ntrunk + k)
    d_tails = (rsup.LhRsBlock * len(tails))(*tails)
    pool = np.full((len(lens), 2, cap_in), 0x7fff, np.int16)
    for s, x in enumerate(pcms):
        pool[s, :, :lens[s]] = x
    if channels == 1 and mix == 0.0:
        pool[:, 1, :] = 0x7fff              # mono without a downmix: the second plane is never read either
    out = np.full((len(lens), 2, cap_out), np.nan, np.float32)
    bank = np.zeros((2 * rs.phases + 1, rsup.LH_RS_ROW), np.float32)
    bank[:, :34] = np.ctypeslib.as_array(rs.bank)[:2 * rs.phases + 1]
    bank[:, rs.taps + 1:] = 0
    p = rsup.LhRsParams()
    p.ratio, p.taps, p.phases, p.channels = rs.ratio, rs.taps, rs.phases, channels
    p.m = rsup.LhRsMatrix(scale, mix, np.float32(0.0) * np.float32(scale), scale_r)
    p.one_plane = int(channels == 1 and mix == 0.0)
    p.cap_in, p.cap_out = cap_in, cap_out
    emu.lh_emu_resample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]
    assert emu.lh_emu_resample(C.byref(p), bank.ctypes.data, trunk.blk, d_tails, streams, len(lens), max_blocks,
                               pool.ctypes.data, out.ctypes.data) == 0
    lib.lh_rs_trunk_free(C.byref(trunk))
    for s, want in enumerate(wants):
        k = want.shape[1]
        assert rsup.same_floats(out[s, :, :k], want), "stream %d" % s
        assert np.isnan(out[s, :, k:]).all(), "stream %d: written beyond its converted length" % s
