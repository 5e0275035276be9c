"""What tests/test_quantizer_identity.py and tests/test_device_leaves.py share: the reference's masking expressions
(psymodel.c:294-341, util.c:976-1001) restated in numpy, and the pair sets they are checked on.  The first file proves
the identities the kernels rely on in numpy, the second that the device evaluates them that way -- on the same pairs."""
import functools

import numpy as np

LOG2_OVER_LOG10 = np.float64(0.69314718055994530942 / 2.30258509299404568402)

# psymodel.c:297-302
TABLE2 = np.array([1.33352 ** 2, 1.35879 ** 2, 1.38454 ** 2, 1.39497 ** 2, 1.40548 ** 2, 1.3537 ** 2, 1.30382 ** 2,
                   1.22321 ** 2, 1.14758 ** 2, 1.0]).astype(np.float32)


def fast_log2(log_table, x):
    """the reference's table-driven log2 of positive normal floats (util.c:976-1001), float32 throughout"""
    bits = x.view(np.uint32)
    mant = (bits & np.uint32(0x7fffff)).astype(np.int32)
    whole = (((bits >> np.uint32(23)) & np.uint32(0xff)).astype(np.int32) - 0x7f).astype(np.float32)
    along = (mant & 16383).astype(np.float32) * np.float32(1.0 / 16384)
    slot = mant >> 14
    return whole + (log_table[slot] * (np.float32(1.0) - along) + log_table[slot + 1] * along)


def mask_cell(log_table, ratio):
    """the reference's table cell for float ratios >= 1 (util.c:976-1001, psymodel.c:331)"""
    lg = fast_log2(log_table, ratio)
    return (lg.astype(np.float64) * (LOG2_OVER_LOG10 * np.float64(16.0))).astype(np.int32)


def boundary(v):
    """midpoint of the float v and its predecessor, in double"""
    below = (np.array([v], np.float32).view(np.uint32) - np.uint32(1)).view(np.float32)[0]
    return 0.5 * (np.float64(v) + np.float64(below))


def far_pairs(rng, c):
    """(larger, smaller) for the rule outside the diagonal band: smaller over every exponent (denormals included) with
    random mantissas and larger = c x smaller +- 0..40 ulps, random pairs, the zero cases"""
    expo = np.repeat(np.arange(0, 254, dtype=np.uint32), 4000)
    lo = ((expo << 23) | rng.integers(0, 1 << 23, expo.size, dtype=np.uint32)).view(np.float32)
    base = (c * lo).astype(np.float32)
    ok = np.isfinite(base)
    lo, base = lo[ok], base[ok]
    hi = (base.view(np.uint32).astype(np.int64) + rng.integers(-40, 41, base.size)).clip(0, 0x7f7fffff).astype(np.uint32).view(np.float32)
    lo2 = rng.random(2_000_000, dtype=np.float32) * np.float32(1e6)
    hi2 = lo2 * (rng.random(2_000_000, dtype=np.float32) * np.float32(2.0) * c)
    lo = np.concatenate([lo, lo2, np.zeros(4, np.float32)])
    hi = np.concatenate([hi, hi2, np.array([0, 1, 1e-40, 3e38], np.float32)])
    return np.maximum(hi, lo), np.minimum(hi, lo)


def far_other_constants(rng):
    """the constants besides ma_max_i2 that the far rule is proved for (drawn before the pairs, from the same generator)"""
    cs = [np.float32(v) for v in (1.0000001, 1.5, 3.1622777, 31.622776, 1000.0)]
    return cs + list(rng.uniform(1.0, 100.0, 8).astype(np.float32))


def far_reference(hi, lo, c):
    """psymodel.c:323-341 behind the `b <= delta' block: is the float quotient below c"""
    return np.where(lo > 0, (hi / lo).astype(np.float32) < c, False)


@functools.lru_cache(maxsize=2)
def _near_walk(table_bytes, c1_bits):
    log_table = np.frombuffer(table_bytes, np.float32)
    lo_b = int(np.float32(1.0).view(np.uint32))
    ratio = np.arange(lo_b, c1_bits, dtype=np.uint32).view(np.float32)
    cell = mask_cell(log_table, ratio)
    steps = ratio[1:][np.diff(cell) != 0]
    return int(cell[0]), int(cell[-1]), bool(np.all(np.diff(cell) >= 0)), steps


def near_walk(log_table, c1):
    """every float ratio in [1, ma_max_i1): first cell, last cell, whether the cell never decreases, the floats it steps at"""
    return _near_walk(np.ascontiguousarray(log_table, np.float32).tobytes(), int(np.float32(c1).view(np.uint32)))


def near_pairs(rng, steps, c1):
    """(a, b) for the rule near the diagonal: pairs around every boundary over the exponent range, random pairs, zeros"""
    los, his = [], []
    for r in list(steps) + [c1]:
        expo = np.repeat(np.arange(0, 250, dtype=np.uint32), 800)
        lo = ((expo << 23) | rng.integers(0, 1 << 23, expo.size, dtype=np.uint32)).view(np.float32)
        base = (np.float32(r) * lo).astype(np.float32)
        ok = np.isfinite(base)
        lo, base = lo[ok], base[ok]
        hi = (base.view(np.uint32).astype(np.int64) + rng.integers(-40, 41, base.size)).clip(0, 0x7f7fffff).astype(np.uint32).view(np.float32)
        los.append(lo)
        his.append(hi)
    lo2 = rng.random(3_000_000, dtype=np.float32) * np.float32(1e6)
    los += [lo2, np.zeros(4, np.float32)]
    his += [lo2 * (rng.random(3_000_000, dtype=np.float32) * np.float32(5.0)), np.array([0, 1, 1e-40, 3e38], np.float32)]
    return np.concatenate(his), np.concatenate(los)


def near_reference(log_table, c1, a, b):
    """psymodel.c:323-333: (a + b) x table2[cell of the quotient], the plain sum from ma_max_i1 on, the other masker at 0"""
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    total = a + b
    q = (hi / np.where(lo > 0, lo, np.float32(1.0))).astype(np.float32)
    safe = np.where((lo > 0) & (q < c1), q, np.float32(1.0))
    return np.where(lo > 0, np.where(q >= c1, total, total * TABLE2[mask_cell(log_table, safe)]), hi)
