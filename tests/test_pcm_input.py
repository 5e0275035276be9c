"""Typed input of a batch without a device: lame_copy_inbuffer's arithmetic as the library's host evaluation
(csrc/lh_pcm_in.h / lh_pcm_in.c) against numpy float32, the SOURCE of the ingest, de-interleave and typed rate
conversion kernels (csrc/lh_ingest.hip, csrc/lh_resample_dev.hip) run by the fiber emulator of tests/hipemu against
that host evaluation bit for bit, and what the binding refuses before it reaches a device."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import lamehip
import pcm_input_support as psup
import resample_support as rsup
from lamehip import PCM_F32, PCM_F32_UNIT, PCM_S16, PCM_S32
from resample_support import FS, MFN

TYPES = [PCM_S32, PCM_F32, PCM_F32_UNIT]
# (name, channels, pcm_scale, pcm_mix, pcm_scale_r, one plane): identity; scale_left 0.7 / scale_right 1.3; stereo to mono
# (the downmix reads both planes); mono from one plane
MATRICES = [("identity", 2, 1.0, 0.0, 1.0, False), ("scales", 2, 0.7, 0.0, 1.3, False), ("downmix", 1, 0.5, 0.5, 0.5, False),
            ("mono", 1, 1.0, 0.0, 1.0, True)]
NORM = {PCM_S32: np.float32(1.0 / 65536.0), PCM_F32: np.float32(1.0), PCM_F32_UNIT: np.float32(32767.0)}
LENGTHS = [0, 1, 3, 4, 5, 1151, 1152, 1153, 5000]


@pytest.fixture(scope="module")
def lib():
    return psup.library()


@pytest.fixture(scope="module")
def emu():
    d = os.path.join(helpers.ROOT, "tests", "hipemu_ingest")
    helpers.locked_make([], d)
    e = C.CDLL(os.path.join(d, "libhipemu_ingest.so"))
    e.lh_emu_ingest.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    e.lh_emu_deinterleave.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    e.lh_emu_resample_typed.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]
    return e


def numpy_ingest(stype, scale, mix, scale_r, left, right):
    """every product and sum a float32 of its own, as lame_copy_inbuffer computes them"""
    f = np.float32
    norm = NORM[stype]
    m00, m01 = norm * f(scale), norm * f(mix)
    m10, m11 = norm * (f(0.0) * f(scale)), norm * f(scale_r)
    assert all(v.dtype == np.float32 for v in (m00, m01, m10, m11))
    xl, xr = left.astype(np.float32), right.astype(np.float32)
    u = (xl * m00).astype(np.float32) + (xr * m01).astype(np.float32)
    v = (xl * m10).astype(np.float32) + (xr * m11).astype(np.float32)
    return np.stack([u, v]).astype(np.float32)


@pytest.mark.parametrize("matrix", MATRICES, ids=[m[0] for m in MATRICES])
@pytest.mark.parametrize("stype", TYPES, ids=[psup.TYPE_NAMES[t] for t in TYPES])
def test_host_evaluation_equals_numpy_float32(stype, matrix, lib):
    _, channels, scale, mix, scale_r, one_plane = matrix
    x = psup.typed_signal(stype, 3100 + stype, 6000)
    if stype == PCM_S32:
        assert (x & 0xffff).any()           # the low 16 bits take part
    else:
        assert (x != np.round(x)).any()     # fractional values
    m = psup.matrix(lib, stype, scale, mix, scale_r)
    got = psup.host_ingest(lib, stype, m, x[0], None if one_plane else x[1])
    want = numpy_ingest(stype, scale, mix, scale_r, x[0], x[0] if one_plane else x[1])
    assert psup.same_floats(got, want)
    # interleaved (stride 2): the same samples, the same floats
    if not one_plane:
        inter = np.ascontiguousarray(x.T)
        assert psup.same_floats(psup.host_ingest(lib, stype, m, None, interleaved=inter), want)
    # -0.0 stays what the arithmetic makes of it: x * 1 + y * 0 is computed, never passed through
    if stype == PCM_F32:
        zl, zr = np.array([-0.0, -0.0, 1.5], np.float32), np.array([1.5, -0.0, -0.0], np.float32)
        got = psup.host_ingest(lib, stype, psup.matrix(lib, stype, 1.0, 0.0, 1.0), zl, zr)
        assert psup.same_floats(got, numpy_ingest(stype, 1.0, 0.0, 1.0, zl, zr))
        assert not np.signbit(got[0][0]) and np.signbit(got[0][1])      # -0 * 1 + 1.5 * 0 = +0, -0 * 1 + -0 * 0 = -0


def aligned_pool(shape, dtype, fill, offset_bytes=0):
    """an array whose first element sits `offset_bytes' behind a 16-byte boundary (a device pool starts on one)"""
    n = int(np.prod(shape))
    raw = np.empty(n * np.dtype(dtype).itemsize + 64, np.uint8)
    at = (-raw.ctypes.data) % 16 + offset_bytes
    a = raw[at:at + n * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
    a[...] = fill
    assert (a.ctypes.data - offset_bytes) % 16 == 0
    return a


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("stype", TYPES, ids=[psup.TYPE_NAMES[t] for t in TYPES])
def test_ingest_kernel_source_matches_host_evaluation(stype, k, lib, emu):
    """lh_ingest_kernel under the emulator: nine ragged streams in rows of 5000 + k elements (k = 0..3: every alignment
    of a row start), the input NaN / 0x7fffffff beyond each length -- and all over the second plane where only one is
    read --, the float pool NaN before: the host evaluation's floats up to each length, NaN beyond, whatever the order
    of the list; a stream that is not on the list stays untouched.  The matrix changes with the case, and one case in
    three has its input pool one element off the float pool's alignment."""
    _, channels, scale, mix, scale_r, one_plane = MATRICES[(k + TYPES.index(stype)) % 4]
    cap = 5000 + k
    dtype = lamehip.PCM_DTYPES[stype]
    m = psup.matrix(lib, stype, scale, mix, scale_r)
    xs = [psup.typed_signal(stype, 3200 + 10 * k + s, n) for s, n in enumerate(LENGTHS)]
    pool = aligned_pool((len(LENGTHS) + 1, 2, cap), dtype, psup.beyond_value(stype), 4 if stype == TYPES[k % 3] else 0)
    wants = []
    for s, x in enumerate(xs):
        pool[s, :, :LENGTHS[s]] = x
        if one_plane:
            pool[s, 1, :] = psup.beyond_value(stype)
        w = psup.host_ingest(lib, stype, m, x[0], None if one_plane else x[1])
        if channels == 1:
            w[1] = 0.0                      # (the rate converter's convention for the second plane of a mono stream)
        wants.append(w)
    p = psup.LhInParams()
    p.m[:] = [float(v) for v in m]
    p.channels, p.one_plane, p.cap = channels, int(one_plane), cap
    outs = []
    for order in (list(range(len(LENGTHS))), [5, 8, 0, 3, 7, 1, 6, 2, 4]):
        out = aligned_pool((len(LENGTHS) + 1, 2, cap), np.float32, np.nan)
        streams = (psup.LhInStream * len(order))(*[psup.LhInStream(LENGTHS[s], s, 0) for s in order])
        assert emu.lh_emu_ingest(stype, C.byref(p), streams, len(order), max(LENGTHS), pool.ctypes.data, out.ctypes.data) == 0
        for s, w in enumerate(wants):
            n = LENGTHS[s]
            assert psup.same_floats(out[s, :, :n], w), "stream %d" % s
            assert np.isnan(out[s, :, n:]).all(), "stream %d: written beyond its length" % s
        assert np.isnan(out[len(LENGTHS)]).all()
        outs.append(out)
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32])
def test_deinterleave_kernel_source(dtype, emu):
    """lh_deinterleave_kernel under the emulator: [n, 2] apart into two rows, nothing written from n on; one plane alone
    when there is no second destination"""
    rng = np.random.default_rng(33)
    esz = np.dtype(dtype).itemsize
    for n in (0, 1, 3, 255, 256, 257, 5000):
        src = rng.integers(-30000, 30000, (n, 2)).astype(dtype)
        for planes in (2, 1):
            dst = np.full((2, n + 7), 77, dtype)
            assert emu.lh_emu_deinterleave(esz, src.ctypes.data, src.ctypes.data + esz, dst[0].ctypes.data,
                                           dst[1].ctypes.data if planes == 2 else None, n) == 0
            assert (dst[0, :n] == src[:, 0]).all() and (dst[:, n:] == 77).all()
            assert (dst[1, :n] == (src[:, 1] if planes == 2 else 77)).all()


@pytest.mark.parametrize("rate_in,rate_out", [(48000, 44100), (96000, 48000)], ids=["31taps", "32taps"])
@pytest.mark.parametrize("stype", [PCM_F32_UNIT, PCM_S32], ids=["f32unit", "s32"])
def test_typed_resample_kernel_source(stype, rate_in, rate_out, lib, emu):
    """lh_resample_kernel with its staging load in the pool's type, under the emulator: the floats of the plan's blocks
    evaluated on the host (csrc/lh_pcm_in.c: lh_pcm_eval_block) over the host-ingested floats"""
    rlib = rsup.library()
    channels, scale, mix, scale_r = 2, 0.8, 0.3, 0.6
    lens = [2 * FS + 401, 0, FS, 700]
    cap_in = max(lens) + 3
    rs = rsup.resampler(rlib, rate_in, rate_out)
    assert rs.taps == (31 if rate_in == 48000 else 32)
    m = psup.matrix(lib, stype, scale, mix, scale_r)
    trunk = rsup.LhRsTrunk()
    rlib.lh_rs_trunk_init(C.byref(trunk), FS, MFN)
    assert rlib.lh_rs_trunk_extend(C.byref(rs), C.byref(trunk), max(lens) // FS) == 0
    xs = [psup.typed_signal(stype, 3300 + s, n, rate_in) for s, n in enumerate(lens)]
    wants = []
    for x in xs:
        n = x.shape[1]
        f = psup.host_ingest(lib, stype, m, x[0], x[1])
        blocks, _, conv, _, _ = rsup.plan(rlib, rs, n)
        w = np.full((2, conv), np.nan, np.float32)
        for b in blocks:
            lib.lh_pcm_eval_block(C.byref(rs), C.byref(b), channels, f[0].ctypes.data, f[1].ctypes.data, n, w[0].ctypes.data,
                                  w[1].ctypes.data)
        assert not np.isnan(w).any()
        wants.append(w)
    cap_out = max(w.shape[1] for w in wants) + 64
    tails, streams, max_blocks = [], (rsup.LhRsStream * len(lens))(), 0
    for s, n in enumerate(lens):
        tail = (rsup.LhRsBlock * 64)()
        conv, frames, padding = C.c_long(0), C.c_int(0), C.c_int(0)
        k = rlib.lh_rs_plan_tail(C.byref(rs), C.byref(trunk), n, tail, 64, C.byref(conv), C.byref(frames), C.byref(padding))
        assert 0 < k <= 64 and conv.value == wants[s].shape[1]
        streams[s] = rsup.LhRsStream(n, s, trunk.after[n // FS].nblk, len(tails), k)
        tails += list(tail[:k])
        max_blocks = max(max_blocks, streams[s].ntrunk + k)
    d_tails = (rsup.LhRsBlock * len(tails))(*tails)
    pool = np.full((len(lens), 2, cap_in), psup.beyond_value(stype), lamehip.PCM_DTYPES[stype])
    for s, x in enumerate(xs):
        pool[s, :, :lens[s]] = x
    out = np.full((len(lens), 2, cap_out), np.nan, np.float32)
    bank = np.zeros((2 * rs.phases + 1, rsup.LH_RS_ROW), np.float32)
    bank[:, :34] = np.ctypeslib.as_array(rs.bank)[:2 * rs.phases + 1]
    bank[:, rs.taps + 1:] = 0
    p = rsup.LhRsParams()
    p.ratio, p.taps, p.phases, p.channels = rs.ratio, rs.taps, rs.phases, channels
    p.m = rsup.LhRsMatrix(*[float(v) for v in m])
    p.one_plane = 0
    p.cap_in, p.cap_out = cap_in, cap_out
    assert emu.lh_emu_resample_typed(stype, C.byref(p), bank.ctypes.data, trunk.blk, d_tails, streams, len(lens), max_blocks,
                                     pool.ctypes.data, out.ctypes.data) == 0
    rlib.lh_rs_trunk_free(C.byref(trunk))
    for s, want in enumerate(wants):
        k = want.shape[1]
        assert psup.same_floats(out[s, :, :k], want), "stream %d" % s
        assert np.isnan(out[s, :, k:]).all(), "stream %d: written beyond its converted length" % s


def test_symbols_are_declared_and_exported():
    lib = lamehip.load_library()
    txt = open(os.path.join(helpers.ROOT, "include", "lamehip.h")).read()
    for name in ("lamehip_batch_set_sample_type", "lamehip_batch_set_input", "lamehip_batch_set_input_device",
                 "lamehip_batch_input_host_ptr", "lamehip_batch_last_ingest_ms"):
        assert name + "(" in txt and hasattr(lib, name), name
    for name in ("LAMEHIP_PCM_S16      0", "LAMEHIP_PCM_S32      1", "LAMEHIP_PCM_F32      2", "LAMEHIP_PCM_F32_UNIT 3"):
        assert "#define " + name in txt
    for name in ("lh_launch_ingest", "lh_launch_deinterleave", "lh_launch_resample_typed", "lh_launch_resample",
                 "lh_pcm_ingest_host"):
        assert hasattr(lib, name), name
    assert (PCM_S16, PCM_S32, PCM_F32, PCM_F32_UNIT) == (0, 1, 2, 3)


class FakeDeviceArray:
    """what the binding asks of an array that lives on the GPU"""
    is_cuda = True

    def __init__(self, dtype, shape):
        self.dtype, self.shape = dtype, shape

    def data_ptr(self):
        raise AssertionError("a refused array is never handed to the library")

    def is_contiguous(self):
        return True


def test_binding_refuses_another_dtype():
    """the dtype must be the batch's: the binding raises before anything reaches the library, and never casts"""
    b = lamehip.Batch.__new__(lamehip.Batch)
    b.b, b.lib = None, None                 # (no device here: a call that got past the check would fail on these)
    x = np.zeros(100, np.float32)
    for stype, bad in ((PCM_S16, x), (PCM_S32, x), (PCM_F32, x.astype(np.float64)), (PCM_F32_UNIT, x.astype(np.int16)),
                       (PCM_F32_UNIT, FakeDeviceArray("torch.float16", (100,)))):
        b.sample_type = stype
        with pytest.raises(TypeError, match="sample type takes"):
            b.set_input(0, bad, bad)
        with pytest.raises(TypeError, match="sample type takes"):
            b.set_input(0, interleaved=bad)
    b.sample_type = PCM_F32
    with pytest.raises(ValueError):
        b.set_input(0, np.zeros((100, 3), np.float32))          # neither planar nor [n, 2]
    with pytest.raises(ValueError):
        b.set_input(0, x, x[:50])
