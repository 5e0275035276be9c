"""Cases, host references and runners of tests/test_device_leaves.py (and of tests/golden/make_leaf_math_golden.py):
the leaf drivers of tests/gpu_tools/lh_leaf_kernels.hip run either on the device (liblamehip_leaftest.so) or on the
CPU (libhipemu_leaf.so: the same source through the fiber emulator), on the same inputs, against the same references.

The specification of a wave primitive is the LH_EMU half of csrc/lh_wave.h, restated here in numpy over arrays of
shape (case, wave, lane)."""
import ctypes as C
import functools
import hashlib
import json
import os
from fractions import Fraction

import numpy as np

import helpers
import identity_support

TOOLS = os.path.join(helpers.ROOT, "tests", "gpu_tools")
DIGESTS = os.path.join(helpers.ROOT, "tests", "golden", "leaf_math_sha256.json")
NT, NIN, NOUT = 128, 8, 24
U32 = np.uint32
ONES = U32(0xffffffff)

# the order of the drivers' `op' (lh_leaf_kernels.hip)
WAVE_OPS = ["sum", "max", "min", "or", "or64", "ballot", "bcast", "maxf", "sum_n", "max_n", "head_tail", "pkmin", "shfl",
            "regions", "max8", "shifts", "above", "sum_maxf", "row0min", "dot2", "ldsread", "bits", "uni", "scans", "dpp",
            "fma", "ldsatom"]
MATH_OPS = ["powf", "logf", "log10f", "adjust", "masklower", "fastlog2", "fastlog2_via", "mask_near", "mask_far",
            "ns_interp", "ldexp"]
LIBM_OPS = {"powf": 0, "logf": 1, "log10f": 2, "adjust": 3, "masklower": 4}

# (slot, control word, row mask, `old'): LEAF_DPP_LIST / LEAF_ROWS_LIST of the driver
DPP_SLOTS = [(0, 0xB1, 0xf, 0), (1, 0x4E, 0xf, 0), (2, 0x141, 0xf, 0), (3, 0x140, 0xf, 0), (4, 0x111, 0xf, 0),
             (5, 0x112, 0xf, 0), (6, 0x113, 0xf, 0), (7, 0x114, 0xf, 0), (8, 0x118, 0xf, 0), (9, 0x128, 0xf, 0),
             (10, 0x104, 0xf, 0), (11, 0x130, 0xf, 0), (12, 0x138, 0xf, 0), (13, 0xB1, 0xf, 0xffffffff),
             (14, 0x4E, 0xf, 0xffffffff), (15, 0x141, 0xf, 0xffffffff), (16, 0x140, 0xf, 0xffffffff),
             (17, 0x138, 0xf, 0x7fffffff), (18, 0x142, 0xa, 0), (19, 0x143, 0xc, 0), (20, 0x142, 0xa, 0xffffffff),
             (21, 0x143, 0xc, 0xffffffff)]

# what each output word of a driver is, for the failure messages
WORDS = {
    "sum": ["lh_wave_sum_u32"], "max": ["lh_wave_max_u32"], "min": ["lh_wave_min_u32"], "or": ["lh_wave_or_u32"],
    "or64": ["lh_wave_or_u64.lo", "lh_wave_or_u64.hi"], "ballot": ["lh_ballot.lo", "lh_ballot.hi"], "bcast": ["lh_bcast_u32"],
    "maxf": ["lh_wave_max_f32"], "sum_n": ["lh_wave_sum_n<3>[0]", "lh_wave_sum_n<3>[1]", "lh_wave_sum_n<3>[2]", "lh_wave_sum_n<1>[0]"],
    "max_n": ["lh_wave_max_n<2>[0]", "lh_wave_max_n<2>[1]"] + ["lh_wave_max_n<4>[%d]" % k for k in range(4)],
    "head_tail": ["lh_wave_sum_head3<2>[0]", "lh_wave_sum_head3<2>[1]", "lh_wave_sum_tail3<2>[0]", "lh_wave_sum_tail3<2>[1]"],
    "pkmin": ["lh_pk_min_u16"], "shfl": ["lh_shfl_u32", "lh_shfl_f32"],
    "regions": ["lh_wave_sum_regions (q total)", "lh_wave_sum_regions *L", "lh_wave_sum_regions *H"], "max8": ["lh_wave_max8"],
    "shifts": ["lh_lane_minus_u32<1>", "lh_lane_minus_u32<2>", "lh_lane_minus_u32<3>", "lh_row_shr_u32<1>", "lh_row_shr_u32<2>",
               "lh_row_shr_u32<4>", "lh_row_shr_u32<8>", "lh_lane_below_u32"],
    "above": ["lh_lane_above_u32"], "sum_maxf": ["lh_wave_sum_maxf *sum", "lh_wave_sum_maxf *mx"], "row0min": ["lh_row0_min_u32"],
    "dot2": ["lh_dot2_u16"], "ldsread": ["lh_lds_read_u32(lh_lds_off)"], "bits": ["lh_popc64", "lh_clz32", "lh_clz64", "lh_ffs64"],
    "uni": ["lh_uni_i", "lh_uni_f", "lh_uni_ll.lo", "lh_uni_ll.hi", "lh_uni_f64.lo", "lh_uni_f64.hi", "lh_vec_u32"],
    "scans": ["lh_wave_scan_u32", "lh_wave_scan_max_u32"],
    "dpp": ["%s<0x%x%s, old 0x%x>" % ("lh_dpp_rows" if m != 0xf else "lh_dpp", c, "/0x%x" % m if m != 0xf else "", o) for _, c, m, o in DPP_SLOTS],
    "fma": ["lh_fma.lo", "lh_fma.hi"], "ldsatom": ["lh_lds_add", "lh_lds_max", "lh_lds_addf"],
}


# ---------------------------------------------------------------------------------------------------- runners
class Runner:
    """the three launchers of one build of the drivers; arrays go in and come back as numpy"""

    def __init__(self, kind):
        self.kind = kind
        name = {"emu": "libhipemu_leaf.so", "gpu": "liblamehip_leaftest.so"}[kind]
        self.lib = C.CDLL(os.path.join(TOOLS, name))
        self.lib.lh_leaf_wave.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self.lib.lh_leaf_bandsum.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
        self.lib.lh_leaf_math.argtypes = [C.c_int, C.c_long] + [C.c_void_p] * 6 + [C.c_int]
        self.sq_n = int(self.lib.lh_leaf_sq_n())
        if kind == "gpu":
            self.lib.lh_leaf_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            self.lib.lh_leaf_free.argtypes = [C.c_void_p]
            self.lib.lh_leaf_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    ERR_SYNC = 10000            # LEAF_ERR_SYNC of the driver: the error came from the wait for the kernel, not from the launch

    def _launched(self, what, rc):
        """a launcher's 0, minus the HIP error of the launch, or minus (ERR_SYNC + the error of the wait for the kernel).  An
        error of the wait is a fault on the device: nothing more is started there, the whole run ends."""
        if self.kind == "gpu":
            for mem in self._live:
                self.lib.lh_leaf_free(mem.ptr)
                mem.ptr = None
            self._live = []
        if rc <= -self.ERR_SYNC and self.kind == "gpu":
            import pytest
            pytest.exit("%s: HIP error %d while waiting for the kernel; no further GPU work is started" % (what, -rc - self.ERR_SYNC), returncode=3)
        assert rc == 0, "%s: launcher returned %d" % (what, rc)

    _live = []

    class _Mem:
        """device memory of one array (allocated by the drivers' own library, so by the HIP runtime that launches)"""

        def __init__(self, lib, nbytes):
            p = C.c_void_p()
            rc = lib.lh_leaf_alloc(C.byref(p), nbytes)
            assert rc == 0 and p.value, "lh_leaf_alloc(%d bytes): HIP error %d" % (nbytes, -rc)
            self.ptr, self.nbytes = p.value, nbytes

    def _dev(self, nbytes):
        m = self._Mem(self.lib, nbytes)
        self._live = self._live + [m]
        return m

    def _in(self, a):
        """-> (pointer, keep-alive)"""
        if a is None:
            return None, None
        a = np.ascontiguousarray(a)
        if self.kind == "emu":
            return a.ctypes.data, a
        m = self._dev(a.nbytes)
        rc = self.lib.lh_leaf_copy(m.ptr, a.ctypes.data, a.nbytes, 1)
        assert rc == 0, "copy to the device: HIP error %d" % -rc
        return m.ptr, m

    def _out(self, nwords):
        a = np.full(nwords, 0x5a5a5a5a, U32)
        if self.kind == "emu":
            return a.ctypes.data, a
        p, m = self._in(a)
        return p, (m, a)

    def _back(self, o):
        """(call before _launched frees the device memory)"""
        if self.kind == "emu":
            return o
        m, a = o
        rc = self.lib.lh_leaf_copy(a.ctypes.data, m.ptr, a.nbytes, 0)
        assert rc == 0, "copy from the device: HIP error %d" % -rc
        return a

    def wave(self, op, x):
        """x: (case, 128, NIN) uint32 -> (case, 128, NOUT) uint32"""
        assert x.dtype == U32 and x.shape[1:] == (NT, NIN)
        pi, ki = self._in(x)
        po, ko = self._out(x.shape[0] * NT * NOUT)
        rc = self.lib.lh_leaf_wave(WAVE_OPS.index(op), x.shape[0], pi, po)
        out = self._back(ko) if rc == 0 else None
        self._launched("lh_leaf_wave(%s)" % op, rc)
        return out.reshape(x.shape[0], NT, NOUT)

    def bandsum(self, pad, sq, n, where):
        assert sq.dtype == np.float32 and sq.shape[1:] == (2, self.sq_n) and n.dtype == np.int32 and where.dtype == np.int32
        ps, ks = self._in(sq)
        pn, kn = self._in(n)
        pw, kw = self._in(where)
        po, ko = self._out(sq.shape[0] * NT * 4)
        rc = self.lib.lh_leaf_bandsum(int(pad), sq.shape[0], ps, pn, pw, po)
        out = self._back(ko) if rc == 0 else None
        self._launched("lh_leaf_bandsum(pad=%d)" % pad, rc)
        return out.reshape(sq.shape[0], NT, 4)

    def math(self, op, a, b=None, c=None, logt=None, mid=None, flag=0):
        a = np.ascontiguousarray(a).view(U32)
        ptrs, keep = [], []
        for arr in (a, None if b is None else np.ascontiguousarray(b).view(U32), None if c is None else np.ascontiguousarray(c).view(U32)):
            p, k = self._in(arr)
            ptrs.append(p)
            keep.append(k)
        po, ko = self._out(a.size)
        pl, kl = self._in(None if logt is None else np.ascontiguousarray(logt, np.float32))
        pm, km = self._in(None if mid is None else np.ascontiguousarray(mid, np.float64))
        rc = self.lib.lh_leaf_math(MATH_OPS.index(op), a.size, ptrs[0], ptrs[1], ptrs[2], po, pl, pm, int(flag))
        out = self._back(ko) if rc == 0 else None
        self._launched("lh_leaf_math(%s)" % op, rc)
        return out


@functools.lru_cache(maxsize=None)
def runner(kind):
    return Runner(kind)


def libm(op, a, b=None, flag=0):
    """the host libm over a sweep (lh_leaf_libm.c, linked into libhipemu_leaf.so)"""
    lib = runner("emu").lib
    lib.lh_leaf_libm.argtypes = [C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    a = np.ascontiguousarray(a).view(U32)
    b = None if b is None else np.ascontiguousarray(b).view(U32)
    out = np.zeros(a.size, U32)
    assert lib.lh_leaf_libm(LIBM_OPS[op], a.size, a.ctypes.data, None if b is None else b.ctypes.data, out.ctypes.data, int(flag)) == 0
    return out


@functools.lru_cache(maxsize=None)
def tables():
    """what the leaves read of LhTables, as numpy"""
    import lamehip
    enc = lamehip.Encoder(44100, 128, require_device=False)
    T = enc.tables()
    t = dict(log_table=np.ctypeslib.as_array(T.log_table).astype(np.float32).copy(),
             mask_mid=np.ctypeslib.as_array(T.mask_mid).astype(np.float64).copy(),
             ma_max_i1=np.float32(T.ma_max_i1), ma_max_i2=np.float32(T.ma_max_i2),
             sfb_l=np.array(list(T.sfb_l)[:23], np.int32),
             pow20=np.ctypeslib.as_array(T.pow20).astype(np.float32).copy(),
             ipow20=np.ctypeslib.as_array(T.ipow20).astype(np.float32).copy())
    enc.close()
    return t


def first_mismatch(leaf, got, want, mask, case_names, extra=""):
    """None, or a message naming the leaf, the case, the wave and lane, with both values in hex"""
    bad = (got != want) & mask
    if not bad.any():
        return None
    c, t = [int(v) for v in np.argwhere(bad)[0]]
    return ("%s: case %s, wave %d lane %d: got 0x%08x, want 0x%08x (%d of %d lanes differ)%s"
            % (leaf, case_names[c], t >> 6, t & 63, int(got[c, t]), int(want[c, t]), int(bad.sum()), int(mask.sum()), extra))


# ---------------------------------------------------------------------------------------------------- wave cases
SINGLE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)


def word_families(rng, nrand=32):
    """[(name, (128, NIN) uint32)]: the inputs every primitive gets -- random full-range words, all zero, all ones, all
    lanes equal, a single non-zero lane at the row edges, the lane index as the value.  The two waves differ."""
    fam = []
    for k in range(nrand):
        fam.append(("random %d" % k, rng.integers(0, 1 << 32, (NT, NIN), dtype=np.uint64).astype(U32)))
    fam.append(("all zero", np.zeros((NT, NIN), U32)))
    fam.append(("all ones", np.full((NT, NIN), ONES, U32)))
    eq = rng.integers(0, 1 << 32, (2, 1, NIN), dtype=np.uint64).astype(U32)
    fam.append(("all lanes equal", np.broadcast_to(eq, (2, 64, NIN)).reshape(NT, NIN).copy()))
    for ln in SINGLE_LANES:
        x = np.zeros((2, 64, NIN), U32)
        x[:, ln, :] = rng.integers(1, 1 << 32, (2, NIN), dtype=np.uint64).astype(U32)
        fam.append(("only lane %d non-zero" % ln, x.reshape(NT, NIN)))
    tid = np.arange(NT, dtype=U32)
    fam.append(("lane index", (tid[:, None] + U32(1) + (np.arange(NIN, dtype=U32)[None, :] << U32(16))).astype(U32)))
    return fam


def float_families(rng, nrand=32):
    """[(name, (128,) float32 bits)]: both signs, +-0, subnormals, +-FLT_MAX; no NaN, no infinity (the stated contract)"""
    fam = []

    def finite(n):
        b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
        e = (b >> U32(23)) & U32(0xff)
        return np.where(e == 0xff, b & U32(0xbfffffff), b).astype(U32)
    for k in range(nrand):
        fam.append(("random floats %d" % k, finite(NT)))
    fam.append(("all +0", np.zeros(NT, U32)))
    fam.append(("all -0", np.full(NT, 0x80000000, U32)))
    fam.append(("+-0 mixed", np.where(rng.integers(0, 2, NT) == 1, U32(0x80000000), U32(0)).astype(U32)))
    fam.append(("all negative", finite(NT) | U32(0x80000000)))
    fam.append(("subnormals of both signs", (finite(NT) & U32(0x807fffff)).astype(U32)))
    fam.append(("negative subnormals and -0", (finite(NT) & U32(0x007fffff)) * (rng.integers(0, 2, NT).astype(U32)) | U32(0x80000000)))
    x = finite(NT)
    x[[5, 100]] = 0x7f7fffff
    x[[6, 90]] = 0xff7fffff
    fam.append(("+-FLT_MAX among random", x))
    fam.append(("all -FLT_MAX", np.full(NT, 0xff7fffff, U32)))
    x = np.full(NT, 0xff7fffff, U32)
    x[[63, 64]] = 0x80000001
    fam.append(("-FLT_MAX and one negative subnormal", x))
    eq = finite(2)
    fam.append(("all lanes equal", np.repeat(eq, 64)))
    for ln in SINGLE_LANES:
        for sign in (0, 0x80000000):
            x = np.zeros(NT, U32)
            v = (finite(2) & U32(0x7fffffff)) | U32(sign)
            x[ln], x[64 + ln] = v[0], v[1]
            fam.append(("only lane %d non-zero (%s)" % (ln, "negative" if sign else "positive"), x))
    fam.append(("lane index", (np.arange(NT) - 40).astype(np.float32).view(U32)))
    return fam


def _stack(fam):
    return [n for n, _ in fam], np.stack([x for _, x in fam]).astype(U32)


def wave_cases(op):
    """(case names, inputs (case, 128, NIN) uint32)"""
    rng = np.random.default_rng(1000 + WAVE_OPS.index(op))
    names, x = _stack(word_families(rng))
    ncase = len(names)
    if op in ("maxf", "sum_maxf"):
        fnames, f = _stack(float_families(rng))
        names = fnames
        x = rng.integers(0, 1 << 32, (len(fnames), NT, NIN), dtype=np.uint64).astype(U32)
        x[:, :, 1 if op == "sum_maxf" else 0] = f
        # the sum beside the maximum: full-range words, and the edge families of the words too
        x[-4:, :, 0 if op == "sum_maxf" else 2] = np.array([0, 0xffffffff, 1, 0x80000000], U32)[:, None]
    elif op == "bcast":
        # every source lane 0..63 (wave 1 reads them in the opposite order), then the families with sources of their own
        more = rng.integers(0, 1 << 32, (64, NT, NIN), dtype=np.uint64).astype(U32)
        for s in range(64):
            more[s, :64, 1] = s
            more[s, 64:, 1] = 63 - s
        for c in range(ncase):
            x[c, :64, 1] = (7 * c + 3) % 64
            x[c, 64:, 1] = (11 * c + 40) % 64
        names = ["source lane %d / %d" % (s, 63 - s) for s in range(64)] + names
        x = np.concatenate([more, x])
    elif op == "shfl":
        lane = np.tile(np.arange(64, dtype=U32), 2)
        src = rng.integers(0, 64, (ncase, NT)).astype(U32)
        special = [("self", lane), ("reversal", U32(63) - lane), ("rotate by 1", (lane + U32(1)) & U32(63)), ("xor 32", lane ^ U32(32))]
        special += [("all lanes read lane %d" % s, np.full(NT, s, U32)) for s in SINGLE_LANES]
        more = rng.integers(0, 1 << 32, (len(special), NT, NIN), dtype=np.uint64).astype(U32)
        more[:, :, 0] += np.arange(NT, dtype=U32)      # (still full range, wraps)
        for k, (_, s) in enumerate(special):
            more[k, :, 1] = s
        x[:, :, 1] = src
        names = ["sources: " + n for n, _ in special] + names
        x = np.concatenate([more, x])
    elif op == "regions":
        # three 10-bit fields of at most 127 per lane, two 16-bit fields of at most 255: "all ones" becomes the maxima
        p = (x[:, :, :3] & U32(127)) | (((x[:, :, :3] >> U32(7)) & U32(127)) << U32(10)) | (((x[:, :, :3] >> U32(14)) & U32(127)) << U32(20))
        q = (x[:, :, 3] & U32(255)) | (((x[:, :, 3] >> U32(8)) & U32(255)) << U32(16))
        x[:, :, :3] = p
        x[:, :, 3] = q
        assert np.all(x[names.index("all ones"), :, :3] == (127 | 127 << 10 | 127 << 20)) and np.all(x[names.index("all ones"), :, 3] == (255 | 255 << 16))
    elif op == "uni":
        # wave-uniform inputs are the contract of lh_uni_*: every lane of a wave holds lane 0's words
        x = np.repeat(x.reshape(ncase, 2, 64, NIN)[:, :, :1, :], 64, axis=2).reshape(ncase, NT, NIN)
    elif op == "fma":
        # three doubles of moderate size; in every second case c = -(a x b) rounded, so that the result is the product's
        # rounding error -- which an unfused multiply-add returns as 0
        man = rng.integers(0, 1 << 52, (ncase, NT, 3), dtype=np.uint64)
        expo = rng.integers(1023 - 30, 1023 + 30, (ncase, NT, 3)).astype(np.uint64)
        sign = rng.integers(0, 2, (ncase, NT, 3)).astype(np.uint64)
        d = ((sign << np.uint64(63)) | (expo << np.uint64(52)) | man).view(np.float64)
        d[1::2, :, 2] = -(d[1::2, :, 0] * d[1::2, :, 1])
        d[2, :, :] = 0.0
        u = d.view(np.uint64)
        x = np.zeros((ncase, NT, NIN), U32)
        x[:, :, 0:6:2] = (u & np.uint64(0xffffffff)).astype(U32)
        x[:, :, 1:6:2] = (u >> np.uint64(32)).astype(U32)
        names = ["doubles %d%s" % (k, " (c = -round(a b))" if k & 1 else "") for k in range(ncase)]
    elif op == "ldsatom":
        x[:, :, 0] = (x[:, :, 0] % U32(2001)).astype(np.int64).astype(np.int32).view(U32) - U32(1000)    # -1000 .. 1000
        x[:, :, 2] = (x[:, :, 2] % U32(1001)).astype(np.float32).view(U32)                               # 0 .. 1000, whole numbers
    elif op == "ldsread":
        x[:8, :, 1] = np.arange(NT, dtype=U32)[::-1]    # (the first cases: a reversal over the workgroup; then random cells)
    return names, x


def dpp_source(ctrl):
    """source lane of every lane for one DPP control word (-1: none)"""
    me = np.arange(64)
    row, r, n = me >> 4, me & 15, ctrl & 15
    if ctrl < 0x100:
        return (me & ~3) | ((ctrl >> (2 * (me & 3))) & 3)
    if 0x101 <= ctrl <= 0x10f:
        return np.where(r + n < 16, me + n, -1)
    if 0x111 <= ctrl <= 0x11f:
        return np.where(r >= n, me - n, -1)
    if 0x121 <= ctrl <= 0x12f:
        return (me & ~15) | ((r - n) & 15)
    return {0x130: np.where(me < 63, me + 1, -1), 0x138: np.where(me > 0, me - 1, -1), 0x140: (me & ~15) | (15 - r),
            0x141: (me & ~7) | (7 - (me & 7)), 0x142: np.where(row > 0, 16 * row - 1, -1), 0x143: np.where(row >= 2, 31, -1)}[ctrl]


def _gather(v, src, fill):
    """v: (..., 64); src: (64,) with -1 = fill"""
    g = v[..., np.where(src < 0, 0, src)]
    return np.where(src < 0, U32(fill), g).astype(U32)


def wave_reference(op, x):
    """x: (case, 128, NIN) -> (want (case, 128, NOUT) uint32, mask of the words that are compared, note per case or None)

    The note marks cases of the float maxima whose result is a zero: lh_wave_max_f32 keeps whichever zero it met first
    (`>' does not order +0 and -0) and lh_wave_sum_maxf's integer key puts +0 above -0, so the sign of a zero maximum is
    not part of the contract; the test compares such a result as a number."""
    ncase = x.shape[0]
    w = x.reshape(ncase, 2, 64, NIN)
    want = np.zeros((ncase, 2, 64, NOUT), U32)
    mask = np.zeros((ncase, 2, 64, NOUT), bool)
    lane = np.arange(64)
    zero_ok = None

    def put(k, v, lanes=None):
        want[..., k] = np.broadcast_to(v, want.shape[:3])
        if lanes is None:
            mask[..., k] = True
        else:
            mask[:, :, lanes, k] = True

    def total(v):
        return (v.astype(np.uint64).sum(axis=2, keepdims=True) & np.uint64(0xffffffff)).astype(U32)

    def fmax(bits):
        f = bits.view(np.float32)
        m = f.max(axis=2, keepdims=True)
        return np.where(m == 0, U32(0), m.view(U32)), (m == 0)

    v = w[..., 0]
    if op == "sum":
        put(0, total(v))
    elif op == "max":
        put(0, v.max(axis=2, keepdims=True))
    elif op == "min":
        put(0, v.min(axis=2, keepdims=True))
    elif op == "or":
        put(0, np.bitwise_or.reduce(v, axis=2, keepdims=True))
    elif op == "or64":
        put(0, np.bitwise_or.reduce(w[..., 0], axis=2, keepdims=True))
        put(1, np.bitwise_or.reduce(w[..., 1], axis=2, keepdims=True))
    elif op == "ballot":
        b = ((v & U32(1)).astype(np.uint64) << lane.astype(np.uint64)).sum(axis=2, keepdims=True)
        put(0, (b & np.uint64(0xffffffff)).astype(U32))
        put(1, (b >> np.uint64(32)).astype(U32))
    elif op == "bcast":
        src = w[:, :, :1, 1].astype(np.int64)
        assert np.all(w[..., 1] == src) and src.max() < 64
        put(0, np.take_along_axis(v, src, axis=2))
    elif op == "maxf":
        m, z = fmax(np.ascontiguousarray(v))
        put(0, m)
        zero_ok = {0: np.broadcast_to(z, want.shape[:3]).reshape(ncase, NT)}
    elif op == "sum_n":
        for k in range(4):
            put(k, total(w[..., k]))
    elif op == "max_n":
        for k in range(6):
            put(k, w[..., k].max(axis=2, keepdims=True))
    elif op == "head_tail":
        for k in range(2):
            g = (w[..., k].reshape(ncase, 2, 8, 8).astype(np.uint64).sum(axis=3, keepdims=True) & np.uint64(0xffffffff)).astype(U32)
            put(k, np.broadcast_to(g, (ncase, 2, 8, 8)).reshape(ncase, 2, 64))
            put(2 + k, total(w[..., k]))
    elif op == "pkmin":
        a, b = w[..., 0], w[..., 1]
        put(0, np.minimum(a & U32(0xffff), b & U32(0xffff)) | (np.minimum(a >> U32(16), b >> U32(16)) << U32(16)))
    elif op == "shfl":
        src = (w[..., 1] & U32(63)).astype(np.int64)
        put(0, np.take_along_axis(w[..., 0], src, axis=2))
        put(1, np.take_along_axis(w[..., 2], src, axis=2))
    elif op == "regions":
        put(0, total(w[..., 3]))
        L = np.zeros((ncase, 2, 64), U32)
        H = np.zeros((ncase, 2, 64), U32)
        for r in range(3):
            p = w[..., r]
            L[:, :, r] = (total(p & U32(0x3ff)) | (total((p >> U32(10)) & U32(0x3ff)) << U32(16)))[:, :, 0]
            H[:, :, r] = total(p >> U32(20))[:, :, 0]
        put(1, L, lanes=[0, 1, 2])      # lane r < 3 returns region r's totals; the other lanes' values are not specified
        put(2, H, lanes=[0, 1, 2])
    elif op == "max8":
        m = w.max(axis=2)               # (case, wave, word)
        put(0, m[:, :, lane & 7])
    elif op == "shifts":
        for k, d in enumerate((1, 2, 3)):
            put(k, _gather(v, np.where((lane & 15) >= d, lane - d, -1), 0))
        for k, d in enumerate((1, 2, 4, 8)):
            put(3 + k, _gather(v, np.where((lane & 15) >= d, lane - d, -1), 0))
        put(7, _gather(v, np.where((lane & 15) >= 1, lane - 1, -1), 0))
    elif op == "above":
        up = np.concatenate([v[:, :, 1:], w[:, :, :1, 1]], axis=2)
        put(0, up)
    elif op == "sum_maxf":
        put(0, total(v))
        m, z = fmax(np.ascontiguousarray(w[..., 1]))
        put(1, m)
        zero_ok = {1: np.broadcast_to(z, want.shape[:3]).reshape(ncase, NT)}
    elif op == "row0min":
        put(0, v[:, :, :16].min(axis=2, keepdims=True))
    elif op == "dot2":
        a, b = w[..., 0], w[..., 1]
        put(0, ((a & U32(0xffff)).astype(np.uint64) * (b & U32(0xffff)) + (a >> U32(16)).astype(np.uint64) * (b >> U32(16)) + w[..., 2]).astype(U32))
    elif op == "ldsread":
        idx = (x[:, :, 1] & U32(NT - 1)).astype(np.int64)
        put(0, np.take_along_axis(x[:, :, 0], idx, axis=1).reshape(ncase, 2, 64))
    elif op == "bits":
        m = w[..., 0].astype(np.uint64) | (w[..., 1].astype(np.uint64) << np.uint64(32))
        bit = ((m[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.int64)       # (..., 64)
        any64, any32 = bit.any(axis=-1), bit[..., :32].any(axis=-1)
        put(0, bit.sum(axis=-1).astype(U32))
        put(1, np.where(any32, np.argmax(bit[..., 31::-1], axis=-1), 32).astype(U32))
        put(2, np.where(any64, np.argmax(bit[..., ::-1], axis=-1), 64).astype(U32))
        put(3, np.where(any64, np.argmax(bit, axis=-1), -1).astype(np.int32).view(U32))
    elif op == "uni":
        for k in range(7):
            put(k, w[..., k])
    elif op == "scans":
        put(0, (np.cumsum(v.astype(np.uint64), axis=2) & np.uint64(0xffffffff)).astype(U32))
        put(1, np.maximum.accumulate(v, axis=2))
    elif op == "dpp":
        row = lane >> 4
        for slot, ctrl, rowmask, old in DPP_SLOTS:
            g = _gather(v, dpp_source(ctrl), 0 if old == 0 else old)    # old = 0 goes with bound_ctrl: no source reads 0
            put(slot, np.where(((rowmask >> row) & 1) == 1, g, U32(old)))
    elif op == "fma":
        u = w[..., 0:6:2].astype(np.uint64) | (w[..., 1:6:2].astype(np.uint64) << np.uint64(32))
        d = u.view(np.float64).reshape(-1, 3)
        r = np.array([float(Fraction(a) * Fraction(b) + Fraction(c)) for a, b, c in d.tolist()], np.float64)
        # (an exact zero: IEEE gives +0 in round-to-nearest unless both addends are -0; Fraction has no sign of zero)
        neg0 = (r == 0) & np.signbit(d[:, 0] * d[:, 1]) & np.signbit(d[:, 2]) & (d[:, 0] * d[:, 1] == 0) & (d[:, 2] == 0)
        r = np.where(neg0, -0.0, r).view(np.uint64).reshape(ncase, 2, 64)
        put(0, (r & np.uint64(0xffffffff)).astype(U32))
        put(1, (r >> np.uint64(32)).astype(U32))
    elif op == "ldsatom":
        s = x[:, :, 0].view(np.int32).astype(np.int64).sum(axis=1).astype(np.int32).view(U32)
        put(0, s[:, None, None])
        put(1, x[:, :, 1].view(np.int32).max(axis=1).view(U32)[:, None, None])
        put(2, x[:, :, 2].view(np.float32).astype(np.float64).sum(axis=1).astype(np.float32).view(U32)[:, None, None])
    else:
        raise KeyError(op)
    return want.reshape(ncase, NT, NOUT), mask.reshape(ncase, NT, NOUT), zero_ok


def check_wave(kind, op):
    names, x = wave_cases(op)
    want, mask, zero_ok = wave_reference(op, x)
    got = runner(kind).wave(op, x)
    assert not mask[:, :, len(WORDS[op]):].any() and mask[:, :, :len(WORDS[op])].any(axis=(0, 1)).all()
    for k, leaf in enumerate(WORDS[op]):
        g, wnt = got[:, :, k].copy(), want[:, :, k]
        if zero_ok is not None and k in zero_ok:
            g = np.where(zero_ok[k] & ((g & U32(0x7fffffff)) == 0), U32(0), g)      # a zero maximum: either sign
        msg = first_mismatch(leaf, g, wnt, mask[:, :, k], names)
        assert msg is None, msg
    return len(names)


# ---------------------------------------------------------------------------------------------------- band sums
WIDTHS_PAD = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 128, 158, 192)
WIDTHS_EVEN = tuple(n for n in WIDTHS_PAD if n % 2 == 0)
BANDSUM_SEED = 20


def serial_sums(terms, n):
    """terms (..., W) float32, n (...,) -> the serial float32 sum of the first n terms, in index order"""
    acc = np.zeros(n.shape, np.float32)
    for i in range(terms.shape[-1]):
        acc = np.where(i < n, acc + terms[..., i], acc).astype(np.float32)
    return acc


def reversed_sums(terms, n):
    acc = np.zeros(n.shape, np.float32)
    for i in range(terms.shape[-1] - 1, -1, -1):
        acc = np.where(i < n, acc + terms[..., i], acc).astype(np.float32)
    return acc


def tree_sums(terms, n):
    """pairwise tree over the first n terms (the rest taken as +0)"""
    W = terms.shape[-1]
    size = 1 << (W - 1).bit_length()
    t = np.zeros(terms.shape[:-1] + (size,), np.float32)
    t[..., :W] = np.where(np.arange(W) < n[..., None], terms, np.float32(0))
    while t.shape[-1] > 1:
        t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
    return t[..., 0]


def bandsum_widths(pad):
    """[(case name, (2, 64) widths)]"""
    rng = np.random.default_rng(BANDSUM_SEED + (1 if pad else 0))
    pool = WIDTHS_PAD if pad else WIDTHS_EVEN
    cases = []
    for k in range(4):
        cases.append(("mixed widths %d" % k, np.stack([np.tile(rng.permutation(pool), 6)[:64] for _ in range(2)])))
    cases.append(("every lane empty", np.zeros((2, 64), np.int64)))
    w = np.zeros((2, 64), np.int64)
    w[0, 0], w[1, 0] = 158, (17 if pad else 16)
    cases.append(("only lane 0", w))
    w = np.zeros((2, 64), np.int64)
    w[0, 63], w[1, 63] = (33 if pad else 32), 192
    cases.append(("only lane 63", w))
    for a, b in ((24, 49 if pad else 48), (8, 16), (32, 1 if pad else 2)):
        cases.append(("all lanes %d / %d wide" % (a, b), np.stack([np.full(64, a), np.full(64, b)])))
    sfb = tables()["sfb_l"]
    long_w = np.zeros(64, np.int64)
    long_w[:22] = np.diff(sfb)
    assert list(long_w[:22]) == [4, 4, 4, 4, 4, 4, 6, 6, 8, 8, 10, 12, 16, 20, 24, 28, 34, 42, 50, 54, 76, 158]
    cases.append(("the 22 long bands at 44.1 kHz", np.stack([long_w, long_w])))
    return cases


@functools.lru_cache(maxsize=None)
def bandsum_cases(pad, sq_n):
    """names, sq (case, 2, sq_n) float32, n (case, 128) int32, where (case, 128) int32, terms (case, 128, 193) float32

    terms: positive, a random mantissa in [1, 4) times one power of two per band; term n of a band is not in the array
    -- it is the `one more term' of the discrimination conditions; the mantissas of a band with n >= 8 are drawn until
    other orders of summation show (see below).  The padded layout: bases on 32-byte boundaries,
    +0.0f up to the next multiple of eight, NaN from there to the end of the band's read-ahead (16 (ceil(n / 16) + 1)
    terms from its base), where the next band starts.  The back-to-back layout: bands in line order from a start that
    is one pair in for every second case, NaN behind the last band."""
    cases = bandsum_widths(pad)
    rng = np.random.default_rng(BANDSUM_SEED + 100 + (1 if pad else 0))
    ncase, W = len(cases), max(WIDTHS_PAD) + 1

    def mantissas(count):
        m = (np.float32(1.0) + rng.integers(0, 3 << 23, (count, W)).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
        return np.minimum(m, np.float32(4.0 - 2.0 ** -21))

    widths = np.stack([wid for _, wid in cases]).reshape(-1)
    man = mantissas(widths.size)
    # A sum in another order agrees with the serial one by chance more often than one would think (for terms of one size
    # the last few additions decide the rounding: 36 % .. 87 % of random bands of 8 .. 192 terms tell a pairwise tree from
    # the serial order, so no seed alone reaches the 90 % asked for).  Every band with n >= 8 therefore draws its mantissas
    # again, from the same distribution, until both a tree sum and a reversed sum differ in bits from its serial sum.
    for _ in range(60):
        right = serial_sums(man, widths).view(U32)
        again = (widths >= 8) & ((tree_sums(man, widths).view(U32) == right) | (reversed_sums(man, widths).view(U32) == right))
        if not again.any():
            break
        man[again] = mantissas(int(again.sum()))
    man = man.reshape(ncase, 2, 64, W)
    scale = np.ldexp(np.float32(1.0), rng.integers(-20, 21, (ncase, 2, 64, 1))).astype(np.float32)
    terms = (man * scale).astype(np.float32)
    assert np.all(man >= 1) and np.all(man < 4)
    sq = np.full((ncase, 2, sq_n), np.nan, np.float32)
    n = np.zeros((ncase, 2, 64), np.int32)
    where = np.zeros((ncase, 2, 64), np.int32)
    for c, (_, wid) in enumerate(cases):
        for wv in range(2):
            pos = 0 if pad else 2 * (c & 1)
            for ln in range(64):
                k = int(wid[wv, ln])
                n[c, wv, ln] = k
                if pad:
                    if k == 0:
                        continue        # (no terms: the lane reads nothing; its base stays 0)
                    where[c, wv, ln] = pos
                    sq[c, wv, pos:pos + k] = terms[c, wv, ln, :k]
                    sq[c, wv, pos + k:pos + (k + 7) // 8 * 8] = 0.0
                    pos += 16 * ((k + 15) // 16 + 1)
                else:
                    where[c, wv, ln] = pos // 2
                    sq[c, wv, pos:pos + k] = terms[c, wv, ln, :k]
                    pos += k
            # the documented read-ahead stays inside the array (the driver checks the same before it calls the leaf)
            if pad:
                assert pos <= sq_n
                assert np.all(where[c, wv] % 8 == 0)
            else:
                maxw = int(n[c, wv].max())
                assert 2 * int(where[c, wv].max()) + 16 * ((maxw + 15) // 16 + 1) <= sq_n
                assert np.all(np.isnan(sq[c, wv, pos:]))
    if not pad:
        jj = where[n > 0]
        assert np.any(jj % 2 == 0) and np.any(jj % 2 == 1), "both even and odd starting pairs must occur"
    used = set(int(v) for v in np.unique(n))
    assert used >= set(WIDTHS_PAD if pad else WIDTHS_EVEN)
    return [nm for nm, _ in cases], sq, n.reshape(ncase, NT), where.reshape(ncase, NT), terms.reshape(ncase, NT, W)


def check_bandsum(kind, pad):
    r = runner(kind)
    names, sq, n, where, terms = bandsum_cases(bool(pad), r.sq_n)
    want = serial_sums(terms, n).view(U32)
    got = r.bandsum(pad, sq, n, where)
    leaf = "lq_band_sums_pad" if pad else "lq_band_sums"
    every = np.ones(n.shape, bool)
    tid = np.arange(NT, dtype=U32)[None, :]
    msg = first_mismatch(leaf + ": marker behind the call (EXEC restored, range check passed)", got[:, :, 1], np.broadcast_to(U32(0xC0DE0000) | tid, n.shape), every, names)
    assert msg is None, msg
    maxw = np.repeat(n.reshape(-1, 2, 64).max(axis=2), 64, axis=1).astype(U32)
    msg = first_mismatch(leaf + ": maxw (lh_wave_max_u32 of n)", got[:, :, 2], maxw, every, names)
    assert msg is None, msg
    extra = ""
    bad = got[:, :, 0] != want
    if bad.any():
        c, t = [int(v) for v in np.argwhere(bad)[0]]
        extra = "; n = %d, first term %d" % (n[c, t], where[c, t] * (1 if pad else 2))
    msg = first_mismatch(leaf, got[:, :, 0], want, every, names, extra)
    assert msg is None, msg
    return len(names)


def bandsum_discrimination(pad, sq_n):
    """the conditions that make the inputs tell a wrong sum from the right one; returns the shares of lanes with n >= 8
    whose pairwise-tree sum / reversed sum differ in bits from the serial sum"""
    names, sq, n, where, terms = bandsum_cases(bool(pad), sq_n)
    assert np.all(terms > 0)
    right = serial_sums(terms, n).view(U32)
    some = n >= 1
    assert np.all((serial_sums(terms, n - 1).view(U32) != right)[some]), "dropping the last term must change every sum"
    assert np.all((serial_sums(terms, n + 1).view(U32) != right)[some]), "one more term must change every sum"
    wide = n >= 8
    tree = float(np.mean((tree_sums(terms, n).view(U32) != right)[wide]))
    rev = float(np.mean((reversed_sums(terms, n).view(U32) != right)[wide]))
    return tree, rev, int(wide.sum())


# ---------------------------------------------------------------------------------------------------- math sweeps
def _f(bits):
    return np.asarray(bits, dtype=np.uint64).astype(U32)


def _both_signs(b):
    return np.concatenate([b, b | U32(0x80000000)])


def _powf_thresholds():
    """2^12 floats either side of the x at which y log2(x) crosses each threshold of lh_powf, at y = 40 (bisection on the
    host in double: the leaf's own log2 differs from it by far less than one of these steps)"""
    y = np.float32(40.0)
    xs = []
    for thr in (126.0, 127.99999995700433, -149.0, -150.0):
        lo, hi = 0x00800000, 0x7f7fffff
        while hi - lo > 1:
            midb = (lo + hi) // 2
            if float(y) * np.log2(float(np.array([midb], U32).view(np.float32)[0])) < thr:
                lo = midb
            else:
                hi = midb
        xs.append(np.arange(hi - 4096, hi + 4096, dtype=np.uint64))
    x = _f(np.concatenate(xs))
    return x, np.full(x.size, y, np.float32).view(U32)


@functools.lru_cache(maxsize=None)
def libm_sweeps():
    """name -> (leaf op, a, b, flag): the sweeps whose authority is the libm of the reference build (glibc 2.35),
    recorded as one sha256 per sweep in tests/golden/leaf_math_sha256.json.  At most 2^24 points each."""
    s = {}
    y = _both_signs(_f(np.arange(0x35000000, 0x42700000, 97, dtype=np.uint64)))
    s["powf(10, y)"] = ("powf", np.full(y.size, np.float32(10.0)).view(U32), y, 0)
    x = np.concatenate([np.arange(1, 0x7f800000, 1013, dtype=np.uint64),
                        np.arange(0x3f800000 - 65536, 0x3f800000 + 65536 + 1, dtype=np.uint64),
                        np.arange(0x00800000 - 65536, 0x00800000 + 65536 + 1, dtype=np.uint64)])
    for nm, r in (("0.36", np.float32(0.6 * float(np.float32(0.6)))), ("0.18", np.float32(0.3 * float(np.float32(0.6))))):
        s["powf(x, %s)" % nm] = ("powf", _f(x), np.full(x.size, r, np.float32).view(U32), 0)
    sx = np.array([0.0, np.inf, 1.0, 1e-45, 3e38], np.float32)
    sy = np.array([0.36, 0.18, -0.5, 0.0, 100.0, -100.0], np.float32)
    s["powf special cases"] = ("powf", np.repeat(sx, sy.size).view(U32), np.tile(sy, sx.size).view(U32), 0)
    tx, ty = _powf_thresholds()
    s["powf thresholds"] = ("powf", tx, ty, 0)
    sub = _f(np.arange(1, 0x00800000, dtype=np.uint64))
    nor = np.concatenate([_f(np.arange(0x00800000, 0x7f800000, 211, dtype=np.uint64)), np.array([0.0, np.inf, 1.0], np.float32).view(U32)])
    for fn in ("logf", "log10f"):
        s[fn + " subnormals"] = (fn, sub, None, 0)
        s[fn + " normals, 0, inf, 1"] = (fn, nor, None, 0)
    pe = np.concatenate([_both_signs(_f(np.arange(0, 0x49800000, 257, dtype=np.uint64))),
                         np.array([0.0, -0.0, 2.0 ** 20, -2.0 ** 20, 3e38, -3e38, np.inf, -np.inf], np.float32).view(U32)])
    s["vbrold_adjust long"] = ("adjust", pe, None, 0)
    s["vbrold_adjust short"] = ("adjust", pe, None, 1)
    s["vbrold_masking_lower"] = ("masklower", _both_signs(_f(np.arange(0, 0x42000000 + 1, 257, dtype=np.uint64))), None, 0)
    for nm, (_, a, _, _) in s.items():
        assert a.size <= 1 << 24, nm
    return s


def sha(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype="<u4").tobytes()).hexdigest()


def committed_digests():
    with open(DIGESTS) as f:
        return json.load(f)


def check_libm_sweep_device(name):
    """device output against the committed digest; on a mismatch the host-compiled leaf locates it"""
    op, a, b, flag = libm_sweeps()[name]
    rec = committed_digests()[name]
    assert rec["points"] == a.size
    got = runner("gpu").math(op, a, b, flag=flag)
    if sha(got) != rec["sha256"]:
        host = runner("emu").math(op, a, b, flag=flag)
        assert sha(host) == rec["sha256"], "%s: the host-compiled leaf does not give the committed digest either" % name
        k = int(np.argwhere(got != host)[0][0])
        raise AssertionError("%s: lh_%s differs from the host-compiled leaf at %d of %d points; first at point %d: a = 0x%08x%s, device 0x%08x, host 0x%08x"
                             % (name, op, int((got != host).sum()), a.size, k, int(a[k]), "" if b is None else ", b = 0x%08x" % int(b[k]), int(got[k]), int(host[k])))
    return a.size


def check_libm_sweep_host(name):
    """libm here == the host-compiled leaf == the committed digest"""
    op, a, b, flag = libm_sweeps()[name]
    rec = committed_digests()[name]
    assert rec["points"] == a.size
    want = libm(op, a, b, flag)
    got = runner("emu").math(op, a, b, flag=flag)
    if not np.array_equal(got, want):
        k = int(np.argwhere(got != want)[0][0])
        raise AssertionError("%s: lh_%s differs from libm at %d of %d points; first at point %d: a = 0x%08x%s, leaf 0x%08x, libm 0x%08x"
                             % (name, op, int((got != want).sum()), a.size, k, int(a[k]), "" if b is None else ", b = 0x%08x" % int(b[k]), int(got[k]), int(want[k])))
    assert sha(want) == rec["sha256"], "%s: this host's libm does not give the committed digest (recorded on glibc 2.35)" % name
    return a.size


def _elementwise(leaf, got, want, ins):
    bad = got != want
    if bad.any():
        k = int(np.argwhere(bad)[0][0])
        raise AssertionError("%s: %d of %d points differ; first at point %d (%s): got 0x%08x, want 0x%08x"
                             % (leaf, int(bad.sum()), got.size, k, ", ".join("0x%08x" % int(np.asarray(v).view(U32)[k]) for v in ins), int(got[k]), int(want[k])))
    return got.size


def check_fast_log2(kind):
    t = tables()
    x = _f(np.arange(0x00800000, 0x7f800000, 211, dtype=np.uint64))
    want = identity_support.fast_log2(t["log_table"], x.view(np.float32)).view(U32)
    n = 0
    for op, leaf in (("fastlog2", "lh_fast_log2"), ("fastlog2_via", "LH_FAST_LOG2_VIA")):
        n += _elementwise(leaf, runner(kind).math(op, x, logt=t["log_table"]), want, [x])
    return n


def check_mask_add(kind):
    t = tables()
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        # far: the pairs test_far_masking_rule_without_the_quotient builds for ma_max_i2 (same generator, same order of draws)
        rng = np.random.default_rng(11)
        identity_support.far_other_constants(rng)
        c2 = t["ma_max_i2"]
        hi, lo = identity_support.far_pairs(rng, c2)
        below = identity_support.far_reference(hi, lo, c2)
        assert identity_support.boundary(c2) == t["mask_mid"][9]
        n = 0
        for m1, m2, order in ((hi, lo, "larger first"), (lo, hi, "smaller first")):
            want = np.where(below, m1 + m2, hi).astype(np.float32).view(U32)      # psymodel.c:336-341
            n += _elementwise("lh_mask_add_far (%s)" % order, runner(kind).math("mask_far", m1, m2, mid=t["mask_mid"]), want, [m1, m2])
        # near: the pairs of test_near_masking_rule_without_quotient_or_logarithm, against the reference's expression
        first, last, monotone, steps = identity_support.near_walk(t["log_table"], t["ma_max_i1"])
        assert len(steps) == 8
        a, b = identity_support.near_pairs(np.random.default_rng(12), steps, t["ma_max_i1"])
        want = identity_support.near_reference(t["log_table"], t["ma_max_i1"], a, b).astype(np.float32).view(U32)
        n += _elementwise("lh_mask_add_near", runner(kind).math("mask_near", a, b, mid=t["mask_mid"]), want, [a, b])
    return n


def check_ns_interp(kind):
    """reference psymodel.c:443-454 with powf = the host-compiled lh_powf (which the libm sweeps tie to libm)"""
    rng = np.random.default_rng(31)
    n = 4096
    x = (rng.random(n, dtype=np.float32) * np.float32(1e6)).astype(np.float32)
    y = (rng.random(n, dtype=np.float32) * np.float32(1e6)).astype(np.float32)
    r = rng.random(n, dtype=np.float32)
    r[:4] = [np.float32(0.6 * float(np.float32(0.6))), np.float32(0.3 * float(np.float32(0.6))), 0.0, 1.0]
    r[rng.integers(0, n, 300)] = np.float32(0.6 * float(np.float32(0.6)))
    r[rng.integers(0, n, 300)] = np.float32(0.3 * float(np.float32(0.6)))
    r[rng.integers(0, n, 200)] = rng.choice(np.array([0.0, -0.0, -0.5, -3e38, 1.0, 1.5, 3e38], np.float32), 200)
    y[rng.integers(0, n, 200)] = 0.0
    x[rng.integers(0, n, 200)] = 0.0
    x[rng.integers(0, n, 100)] = np.float32(1e-30)
    y[rng.integers(0, n, 100)] = np.float32(1e30)
    with np.errstate(all="ignore"):
        q = (x / np.where(y > 0, y, np.float32(1.0))).astype(np.float32)
        p = runner("emu").math("powf", q, r).view(np.float32)
        want = np.where(r >= 1, x, np.where(r <= 0, y, np.where(y > 0, (p * y).astype(np.float32), np.float32(0)))).astype(np.float32).view(U32)
    assert np.sum(r <= 0) >= 50 and np.sum(r >= 1) >= 50 and np.sum(y == 0) >= 50
    return _elementwise("lh_ns_interp", runner(kind).math("ns_interp", x, y, r), want, [x, y, r])


def check_ldexp(kind):
    """the four pow20 and sixteen ipow20 mantissas the search rebuilds its step tables from (lh_dev_qloop.h), times every
    exponent that keeps the result normal; the exponent is the same over each run of 64 points (wave-uniform)"""
    t = tables()
    man = np.concatenate([t["pow20"][210 + 116:214 + 116], t["ipow20"][210:226]]).astype(np.float32)
    assert man.size == 20 and np.all(man > 0)
    row = np.resize(man, 64)
    mexp = np.frexp(row)[1] - 1                 # row = m x 2^mexp, 1 <= m < 2
    es = np.arange(-126 - int(mexp.max()), 127 - int(mexp.min()) + 1)
    v, e = [], []
    for k in es:
        keep = (mexp + k >= -126) & (mexp + k <= 127)
        if keep.any():
            v.append(np.where(keep, row, row[keep][0]))
            e.append(np.full(64, k, np.int32))
    v, e = np.concatenate(v).astype(np.float32), np.concatenate(e)
    want = np.ldexp(v, e).astype(np.float32)
    assert np.all(np.isfinite(want)) and np.all(want.view(U32) >= 0x00800000) and v.size >= 64 * 250
    return _elementwise("lq_ldexp", runner(kind).math("ldexp", v, e.view(U32)), want.view(U32), [v, e.view(U32)])
