"""Typed and device-resident appends of an incremental batch without a device: the SOURCE of the append kernel
(csrc/lh_ingest.hip: lh_append_kernel) run by the fiber emulator of tests/hipemu against the library's host evaluation of
lame_copy_inbuffer's arithmetic (csrc/lh_pcm_in.c) bit for bit, the new names in the header and among the library's
exports, and what the binding refuses before it reaches a device."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import lamehip
import pcm_input_support as psup
from lamehip import PCM_F32, PCM_F32_UNIT, PCM_S16, PCM_S32

TYPES = [PCM_S32, PCM_F32, PCM_F32_UNIT, PCM_S16]
# (name, channels, pcm_scale, pcm_mix, pcm_scale_r, one plane): the four of tests/test_pcm_input.py
MATRICES = [("identity", 2, 1.0, 0.0, 1.0, False), ("scales", 2, 0.7, 0.0, 1.3, False), ("downmix", 1, 0.5, 0.5, 0.5, False),
            ("mono", 1, 1.0, 0.0, 1.0, True)]
LENGTHS = [0, 1, 3, 4, 5, 7, 255, 256, 257, 1151, 1152, 1153, 4099]
POOL_BEFORE = {PCM_S16: -21846}             # (any other type: NaN)


class LhApSeg(C.Structure):
    """csrc/lh_pcm_in.h"""
    _fields_ = [("l", C.c_ulonglong), ("r", C.c_ulonglong), ("at", C.c_longlong), ("n", C.c_longlong), ("stream", C.c_int),
                ("stride", C.c_int)]


@pytest.fixture(scope="module")
def lib():
    return psup.library()


@pytest.fixture(scope="module")
def emu():
    d = os.path.join(helpers.ROOT, "tests", "hipemu_ingest")
    helpers.locked_make([], d)
    e = C.CDLL(os.path.join(d, "libhipemu_ingest.so"))
    e.lh_emu_append.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
    return e


def aligned_pool(shape, dtype, fill, offset_bytes=0):
    """an array whose first element sits `offset_bytes' behind a 16-byte boundary (as in tests/test_pcm_input.py)"""
    n = int(np.prod(shape))
    raw = np.empty(n * np.dtype(dtype).itemsize + 64, np.uint8)
    at = (-raw.ctypes.data) % 16 + offset_bytes
    a = raw[at:at + n * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
    a[...] = fill
    assert (a.ctypes.data - offset_bytes) % 16 == 0
    return a


def source(stype, x, stride, one_plane, off_l, off_r):
    """the samples x [2, n] as a segment's source, the type's beyond_value around them (and all over the right plane where
    only one is read): the addresses of the first left and right sample -- off_l / off_r bytes behind a 16-byte boundary
    -- and what has to stay alive"""
    dtype = lamehip.PCM_DTYPES[stype]
    esz, beyond, n = dtype.itemsize, psup.beyond_value(stype), x.shape[1]
    pad = 16 // esz                         # (a whole 16 bytes in front: the first sample keeps the buffer's offset)
    if stride == 2:
        buf = aligned_pool((n + 2 * pad, 2), dtype, beyond, off_l)
        buf[pad:pad + n, 0] = x[0]
        if not one_plane:
            buf[pad:pad + n, 1] = x[1]
        first = buf.ctypes.data + 2 * pad * esz
        assert first % 16 == off_l
        return first, first + esz, (buf,)
    left, right = aligned_pool((n + 2 * pad,), dtype, beyond, off_l), aligned_pool((n + 2 * pad,), dtype, beyond, off_r)
    left[pad:pad + n] = x[0]
    if not one_plane:
        right[pad:pad + n] = x[1]
    assert (left.ctypes.data + pad * esz) % 16 == off_l and (right.ctypes.data + pad * esz) % 16 == off_r
    return left.ctypes.data + pad * esz, right.ctypes.data + pad * esz, (left, right)


def expected(lib, stype, m, x, channels, one_plane):
    """what positions [at, at + n) of the pool's two rows hold afterwards"""
    if stype == PCM_S16:
        return np.stack([x[0], x[0] if one_plane else x[1]])
    w = psup.host_ingest(lib, stype, m, x[0], None if one_plane else x[1])
    if channels == 1:
        w[1] = 0.0                          # (the convention of the ingest for the second plane of a mono stream)
    return w


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("stype", TYPES, ids=[psup.TYPE_NAMES[t] for t in TYPES])
def test_append_kernel_source_matches_host_evaluation(stype, k, lib, emu):
    """lh_append_kernel under the emulator, pool rows of 5000 + k elements.  One segment per length of LENGTHS, each in a
    stream of its own at a position whose residue mod 4 changes from one to the next, stride 1 and 2 in turn, its sources
    0, 4, 8 or 12 bytes behind a 16-byte boundary (s16: 2 more for every other one); a stream with two segments back to
    back; a stream with none.  The pool is NaN before (s16: a marker), the sources hold the type's beyond_value outside
    the segment -- and all over the right plane where one plane is read: the host evaluation's floats (s16: the samples)
    inside every [at, at + n), untouched everywhere else, byte-identical pools for two orders of the table."""
    _, channels, scale, mix, scale_r, one_plane = MATRICES[(k + TYPES.index(stype)) % 4]
    cap = 5000 + k
    dtype = np.dtype(np.int16) if stype == PCM_S16 else np.dtype(np.float32)
    before = POOL_BEFORE.get(stype, np.nan)
    m = psup.matrix(lib, stype if stype != PCM_S16 else PCM_F32, scale, mix, scale_r)
    # (stream, at, n, stride, offset of the left source, of the right source)
    table = []
    for i, n in enumerate(LENGTHS):
        odd = 2 * (i % 2) if stype == PCM_S16 else 0
        table.append((i, 3 + 5 * i, n, 1 + (i + k) % 2, 4 * ((i // 2 + k) % 4) + odd, 4 * ((i // 2 + k + i % 3) % 4) + odd))
    two = len(LENGTHS)
    table.append((two, 2 + k, 257, 1, 8, 0))
    table.append((two, 2 + k + 257, 1153, 2, 4, 8))
    nstreams = two + 2                      # (the last one has no segment)
    assert {t[1] % 4 for t in table} == {0, 1, 2, 3} and {t[3] for t in table} == {1, 2}
    assert {t[4] for t in table} >= {0, 4, 8, 12} and all(t[1] + t[2] <= cap for t in table)
    for stride in (1, 2):
        assert {t[4] & ~3 for t in table if t[3] == stride} == {0, 4, 8, 12}
    segs, wants, keep = [], [], []
    for j, (s, at, n, stride, off_l, off_r) in enumerate(table):
        x = psup.typed_signal(stype, 4200 + 100 * k + j, n)
        pl, pr, held = source(stype, x, stride, one_plane, off_l, off_r)
        keep.append(held)
        segs.append(LhApSeg(pl, pr, at, n, s, stride))
        wants.append(expected(lib, stype, m, x, channels, one_plane))
    p = psup.LhInParams()
    p.m[:] = [float(v) for v in m]
    p.channels, p.one_plane, p.cap = channels, int(one_plane), cap
    order2 = [9, 14, 0, 12, 3, 7, 13, 1, 6, 11, 2, 10, 4, 8, 5]
    assert sorted(order2) == list(range(len(table)))
    pools = []
    for order in (list(range(len(table))), order2):
        pool = aligned_pool((nstreams, 2, cap), dtype, before)
        arr = (LhApSeg * len(order))(*[segs[j] for j in order])
        assert emu.lh_emu_append(stype, C.byref(p), arr, len(order), max(LENGTHS), pool.ctypes.data) == 0
        untouched = np.ones(pool.shape, bool)
        for j, (s, at, n, _, _, _) in enumerate(table):
            assert psup.same_floats(np.ascontiguousarray(pool[s, :, at:at + n]), wants[j].astype(dtype)), "segment %d" % j
            untouched[s, :, at:at + n] = False
        rest = pool[untouched]
        assert (np.isnan(rest) if stype != PCM_S16 else rest == before).all(), "written outside the segments"
        assert untouched[nstreams - 1].all()
        pools.append(pool)
    assert pools[0].tobytes() == pools[1].tobytes()


def test_append_symbols_are_declared_and_exported():
    lib = lamehip.load_library()
    txt = open(os.path.join(helpers.ROOT, "include", "lamehip.h")).read()
    for name in ("lamehip_batch_append_input", "lamehip_batch_append_input_device", "lamehip_batch_append_device",
                 "lamehip_batch_last_append_ms"):
        assert name + "(" in txt and hasattr(lib, name), name
    assert hasattr(lib, "lh_launch_append")


class FakeDeviceArray:
    """what the binding asks of an array that lives on the GPU"""
    is_cuda = True

    def __init__(self, dtype, shape, strides=None):
        self.dtype, self.shape = dtype, tuple(shape)
        if strides is None:
            strides, step = [], 1
            for d in reversed(self.shape):
                strides.insert(0, step)
                step *= d
        self._strides = tuple(strides)

    def stride(self, d=None):
        return self._strides if d is None else self._strides[d]

    def data_ptr(self):
        raise AssertionError("a refused array is never handed to the library")

    def is_contiguous(self):
        return True


def unopened_batch(stype, nstreams=3, channels=2):
    b = lamehip.Batch.__new__(lamehip.Batch)
    b.b, b.lib = None, None                 # (no device here: a call that got past the checks would fail on these)
    b.n, b.sample_type = nstreams, stype
    b.enc = type("E", (), {"channels": channels})()
    return b


def test_binding_refuses_another_dtype_or_shape():
    """append_input / append_device: the dtype must be the batch's and the shape one of those documented -- the binding
    raises before anything reaches the library, and never casts"""
    x = np.zeros(100, np.float32)
    for stype, bad in ((PCM_S16, x), (PCM_S32, x), (PCM_F32, x.astype(np.float64)), (PCM_F32_UNIT, x.astype(np.int16)),
                       (PCM_F32_UNIT, FakeDeviceArray("torch.float16", (100,)))):
        b = unopened_batch(stype)
        with pytest.raises(TypeError, match="sample type takes"):
            b.append_input(0, bad, bad)
        with pytest.raises(TypeError, match="sample type takes"):
            b.append_input(0, interleaved=bad)
    b = unopened_batch(PCM_F32)
    with pytest.raises(ValueError):
        b.append_input(0, np.zeros((100, 3), np.float32))       # neither planar nor [n, 2]
    with pytest.raises(ValueError):
        b.append_input(0, x, x[:50])
    with pytest.raises(ValueError):
        b.append_input(0, x, interleaved=np.zeros((100, 2), np.float32))
    # append_device: a device array of the batch's dtype, [B, 2, T], [B, T] or [B, T, 2], one length per stream
    lengths = [10, 0, 7]
    with pytest.raises(TypeError, match="sample type takes"):
        b.append_device(FakeDeviceArray("torch.float16", (3, 2, 50)), lengths)
    with pytest.raises(TypeError, match="device array"):
        b.append_device(np.zeros((3, 2, 50), np.float32), lengths)
    for shape in ((3, 3, 50), (2, 2, 50), (3,), (3, 2, 50, 1)):
        with pytest.raises(ValueError):
            b.append_device(FakeDeviceArray("torch.float32", shape), lengths)
    with pytest.raises(ValueError):
        b.append_device(FakeDeviceArray("torch.float32", (3, 2, 50)), [10, 0])          # a length per stream
    with pytest.raises(ValueError):
        b.append_device(FakeDeviceArray("torch.float32", (3, 2, 50)), [10, 51, 0])      # more than the array holds
    with pytest.raises(ValueError):
        b.append_device(FakeDeviceArray("torch.float32", (3, 2, 50)), [10, -1, 0])
    with pytest.raises(ValueError):
        b.append_device(FakeDeviceArray("torch.float32", (3, 2, 50), (200, 100, 2)), lengths)   # samples two apart
    with pytest.raises(ValueError):
        b.append_device(FakeDeviceArray("torch.float32", (3, 50)), lengths)             # [B, T] on a stereo batch
