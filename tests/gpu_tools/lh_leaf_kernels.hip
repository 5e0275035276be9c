/*
 * lh_leaf_kernels.hip -- TEST TOOL (not part of liblamehip): drivers for the device-only leaves the kernels are
 * built from -- the cross-lane primitives of lh_wave.h, the two scans of lh_dev_common.h, the DPP control words the
 * code base uses, the hand-written band sums of lh_dev_qloop.h and the math leaves of lh_dev_math.h /
 * lh_dev_psy_core.h / lh_dev_qloop.h.  A driver takes input arrays, applies one leaf per lane per case and writes
 * every lane's result to an output array; tests/test_device_leaves.py compares on the host.
 *
 * The file is compiled twice by tests/gpu_tools/Makefile: by hipcc for gfx950 with the product's KOPT and STRICT
 * (liblamehip_leaftest.so: the code that ships), and by g++ with -DLH_EMU against tests/hipemu (libhipemu_leaf.so:
 * the same cases on a CPU, which proves the cases and the host references without a GPU).  The product headers are
 * included exactly as csrc/lh_kernels.hip includes them.
 */
#include <stdint.h>
#include <math.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_CONST static const
#else
#include <hip/hip_runtime.h>
#define LH_CONST __device__ static const
#endif

#ifdef LH_EMU
#include <string.h>
#endif
#include "lh_static_tables.h"
#include "lh_dev_common.h"
#include "lh_dev_psy.h"
#include "lh_dev_mdct.h"
#include "lh_dev_quant.h"
#include "lh_dev_qloop.h"

#define LEAF_NT 128             /* two waves per workgroup, as in the product */
#define LEAF_NIN 8              /* input words per lane and case */
#define LEAF_NOUT 24            /* output words per lane and case */

/* ---- DPP control words, at the bound_ctrl settings the code base uses them with ------------------------------------
 * (slot, control word, `old' operand): old = 0 goes with bound_ctrl, anything else without (lh_dpp in lh_wave.h).
 * 0x138 with 0 / 0x7fffffff and 0x130 with 0 are the raw uses in lh_dev_quant.h. */
#define LEAF_DPP_LIST(X) \
    X(0, 0xB1, 0u) X(1, 0x4E, 0u) X(2, 0x141, 0u) X(3, 0x140, 0u) X(4, 0x111, 0u) X(5, 0x112, 0u) X(6, 0x113, 0u) \
    X(7, 0x114, 0u) X(8, 0x118, 0u) X(9, 0x128, 0u) X(10, 0x104, 0u) X(11, 0x130, 0u) X(12, 0x138, 0u) \
    X(13, 0xB1, 0xffffffffu) X(14, 0x4E, 0xffffffffu) X(15, 0x141, 0xffffffffu) X(16, 0x140, 0xffffffffu) \
    X(17, 0x138, 0x7fffffffu)
#define LEAF_ROWS_LIST(X) \
    X(18, 0x142, 0xa, 0u) X(19, 0x143, 0xc, 0u) X(20, 0x142, 0xa, 0xffffffffu) X(21, 0x143, 0xc, 0xffffffffu)

#ifdef LH_EMU
/* what the control words mean, restated for the CPU build (lane -> source lane; no source: 0 with bound_ctrl, else `old') */
static inline uint32_t
leaf_dpp_emu(int ctrl, int rowmask, int bound_ctrl, uint32_t old, uint32_t v)
{
    const uint64_t *x = hipemu_wave_exchange(v);
    int const me = lh_lane(), row = me >> 4, r = me & 15, n = ctrl & 15;
    int     src = -1;
    if (ctrl < 0x100)
        src = (me & ~3) | ((ctrl >> (2 * (me & 3))) & 3);       /* quad_perm */
    else if (ctrl >= 0x101 && ctrl <= 0x10f)
        src = (r + n < 16) ? me + n : -1;       /* row_shl */
    else if (ctrl >= 0x111 && ctrl <= 0x11f)
        src = (r >= n) ? me - n : -1;   /* row_shr */
    else if (ctrl >= 0x121 && ctrl <= 0x12f)
        src = (me & ~15) | ((r - n) & 15);      /* row_ror */
    else if (ctrl == 0x130)
        src = (me < 63) ? me + 1 : -1;  /* wave_shl:1 */
    else if (ctrl == 0x138)
        src = (me > 0) ? me - 1 : -1;   /* wave_shr:1 */
    else if (ctrl == 0x140)
        src = (me & ~15) | (15 - r);    /* row_mirror */
    else if (ctrl == 0x141)
        src = (me & ~7) | (7 - (me & 7));       /* row_half_mirror */
    else if (ctrl == 0x142)
        src = (row > 0) ? 16 * row - 1 : -1;    /* row_bcast:15 */
    else if (ctrl == 0x143)
        src = (row >= 2) ? 31 : -1;     /* row_bcast:31 */
    if (!((rowmask >> row) & 1))
        return old;
    if (src < 0)
        return bound_ctrl ? 0u : old;
    return (uint32_t) x[src];
}
#define LEAF_DPP(slot, ctrl, ident) o[slot] = leaf_dpp_emu(ctrl, 0xf, (ident) == 0u, ident, v);
#define LEAF_ROWS(slot, ctrl, mask, ident) o[slot] = leaf_dpp_emu(ctrl, mask, 0, ident, v);
#else
#define LEAF_DPP(slot, ctrl, ident) o[slot] = lh_dpp < ctrl, ident > (v);
#define LEAF_ROWS(slot, ctrl, mask, ident) o[slot] = lh_dpp_rows < ctrl, mask, ident > (v);
#endif

enum {
    LEAF_W_SUM = 0, LEAF_W_MAX, LEAF_W_MIN, LEAF_W_OR, LEAF_W_OR64, LEAF_W_BALLOT, LEAF_W_BCAST, LEAF_W_MAXF,
    LEAF_W_SUM_N, LEAF_W_MAX_N, LEAF_W_HEAD_TAIL, LEAF_W_PKMIN, LEAF_W_SHFL, LEAF_W_REGIONS, LEAF_W_MAX8,
    LEAF_W_SHIFTS, LEAF_W_ABOVE, LEAF_W_SUM_MAXF, LEAF_W_ROW0MIN, LEAF_W_DOT2, LEAF_W_LDSREAD, LEAF_W_BITS,
    LEAF_W_UNI, LEAF_W_SCANS, LEAF_W_DPP, LEAF_W_FMA, LEAF_W_LDSATOM, LEAF_W_NOPS
};

/* one case per workgroup: in[(case * 128 + thread) * LEAF_NIN + k], out[(case * 128 + thread) * LEAF_NOUT + k] */
LH_DEVFN void
leaf_wave_body(int op, const uint32_t *in, uint32_t *out)
{
    __shared__ uint32_t cell[LEAF_NT];
    __shared__ int acc[2];
    __shared__ float accf[1];
    int const tid = (int) threadIdx.x;
    long const at = (long) blockIdx.x * LEAF_NT + tid;
    uint32_t i[LEAF_NIN], o[LEAF_NOUT];
    for (int k = 0; k < LEAF_NIN; k++)
        i[k] = in[at * LEAF_NIN + k];
    for (int k = 0; k < LEAF_NOUT; k++)
        o[k] = 0u;
    uint32_t const v = i[0];
    switch (op) {
    case LEAF_W_SUM:
        o[0] = lh_wave_sum_u32(v);
        break;
    case LEAF_W_MAX:
        o[0] = lh_wave_max_u32(v);
        break;
    case LEAF_W_MIN:
        o[0] = lh_wave_min_u32(v);
        break;
    case LEAF_W_OR:
        o[0] = lh_wave_or_u32(v);
        break;
    case LEAF_W_OR64: {
            uint64_t const r = lh_wave_or_u64((uint64_t) i[0] | ((uint64_t) i[1] << 32));
            o[0] = (uint32_t) r;
            o[1] = (uint32_t) (r >> 32);
        }
        break;
    case LEAF_W_BALLOT: {
            uint64_t const r = lh_ballot((int) (v & 1u));
            o[0] = (uint32_t) r;
            o[1] = (uint32_t) (r >> 32);
        }
        break;
    case LEAF_W_BCAST:
        o[0] = lh_bcast_u32(v, lh_uni_i((int) i[1]));
        break;
    case LEAF_W_MAXF:
        o[0] = lh_f32_as_u32(lh_wave_max_f32(lh_u32_as_f32(v)));
        break;
    case LEAF_W_SUM_N: {
            uint32_t a[3] = { i[0], i[1], i[2] }, b[1] = { i[3] };
            lh_wave_sum_n < 3 > (a);
            lh_wave_sum_n < 1 > (b);
            o[0] = a[0];
            o[1] = a[1];
            o[2] = a[2];
            o[3] = b[0];
        }
        break;
    case LEAF_W_MAX_N: {
            uint32_t a[2] = { i[0], i[1] }, b[4] = { i[2], i[3], i[4], i[5] };
            lh_wave_max_n < 2 > (a);
            lh_wave_max_n < 4 > (b);
            o[0] = a[0];
            o[1] = a[1];
            o[2] = b[0];
            o[3] = b[1];
            o[4] = b[2];
            o[5] = b[3];
        }
        break;
    case LEAF_W_HEAD_TAIL: {
            uint32_t a[2] = { i[0], i[1] };
            lh_wave_sum_head3 < 2 > (a);
            o[0] = a[0];
            o[1] = a[1];
            lh_wave_sum_tail3 < 2 > (a);
            o[2] = a[0];
            o[3] = a[1];
        }
        break;
    case LEAF_W_PKMIN:
        o[0] = lh_pk_min_u16(i[0], i[1]);
        break;
    case LEAF_W_SHFL:
        o[0] = lh_shfl_u32(v, (int) i[1]);
        o[1] = lh_f32_as_u32(lh_shfl_f32(lh_u32_as_f32(i[2]), (int) i[1]));
        break;
    case LEAF_W_REGIONS: {
            uint32_t L = 0, H = 0;
            o[0] = lh_wave_sum_regions(i[0], i[1], i[2], i[3], &L, &H);
            o[1] = L;
            o[2] = H;
        }
        break;
    case LEAF_W_MAX8: {
            uint32_t const w[8] = { i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7] };
            o[0] = lh_wave_max8(w);
        }
        break;
    case LEAF_W_SHIFTS:
        o[0] = lh_lane_minus_u32 < 1 > (v);
        o[1] = lh_lane_minus_u32 < 2 > (v);
        o[2] = lh_lane_minus_u32 < 3 > (v);
        o[3] = lh_row_shr_u32 < 1 > (v);
        o[4] = lh_row_shr_u32 < 2 > (v);
        o[5] = lh_row_shr_u32 < 4 > (v);
        o[6] = lh_row_shr_u32 < 8 > (v);
        o[7] = lh_lane_below_u32(v);
        break;
    case LEAF_W_ABOVE:
        o[0] = lh_lane_above_u32(i[0], i[1]);
        break;
    case LEAF_W_SUM_MAXF: {
            int     s = 0;
            float   m = 0.0f;
            lh_wave_sum_maxf(i[0], lh_u32_as_f32(i[1]), &s, &m);
            o[0] = (uint32_t) s;
            o[1] = lh_f32_as_u32(m);
        }
        break;
    case LEAF_W_ROW0MIN:
        o[0] = lh_row0_min_u32(v);
        break;
    case LEAF_W_DOT2:
#ifdef LH_EMU
        o[0] = (i[0] & 0xffffu) * (i[1] & 0xffffu) + (i[0] >> 16) * (i[1] >> 16) + i[2];        /* (no CPU half in lh_wave.h) */
#else
        o[0] = lh_dot2_u16(i[0], i[1], i[2]);
#endif
        break;
    case LEAF_W_LDSREAD:
        cell[tid] = v;
        __syncthreads();
#ifdef LH_EMU
        o[0] = cell[i[1] & (LEAF_NT - 1)];      /* (no CPU half in lh_wave.h) */
#else
        o[0] = lh_lds_read_u32(lh_lds_off(&cell[i[1] & (LEAF_NT - 1)]));
#endif
        break;
    case LEAF_W_BITS: {
            uint64_t const m = (uint64_t) i[0] | ((uint64_t) i[1] << 32);
            o[0] = (uint32_t) lh_popc64(m);
            o[1] = (uint32_t) lh_clz32(i[0]);
            o[2] = (uint32_t) lh_clz64(m);
            o[3] = (uint32_t) lh_ffs64(m);
        }
        break;
    case LEAF_W_UNI: {
            /* (inputs are wave-uniform, which is the contract of lh_uni_*) */
            long long const ll = lh_uni_ll((long long) ((uint64_t) i[2] | ((uint64_t) i[3] << 32)));
            uint64_t const d = lh_f64_as_u64(lh_uni_f64(lh_u64_as_f64((uint64_t) i[4] | ((uint64_t) i[5] << 32))));
            o[0] = (uint32_t) lh_uni_i((int) i[0]);
            o[1] = lh_f32_as_u32(lh_uni_f(lh_u32_as_f32(i[1])));
            o[2] = (uint32_t) (uint64_t) ll;
            o[3] = (uint32_t) ((uint64_t) ll >> 32);
            o[4] = (uint32_t) d;
            o[5] = (uint32_t) (d >> 32);
            o[6] = lh_vec_u32(i[6]);
        }
        break;
    case LEAF_W_SCANS:
        o[0] = lh_wave_scan_u32(v);
        o[1] = lh_wave_scan_max_u32(v);
        break;
    case LEAF_W_DPP:
        LEAF_DPP_LIST(LEAF_DPP)
        LEAF_ROWS_LIST(LEAF_ROWS)
        break;
    case LEAF_W_FMA: {
            uint64_t const r = lh_f64_as_u64(lh_fma(lh_u64_as_f64((uint64_t) i[0] | ((uint64_t) i[1] << 32)),
                                                    lh_u64_as_f64((uint64_t) i[2] | ((uint64_t) i[3] << 32)),
                                                    lh_u64_as_f64((uint64_t) i[4] | ((uint64_t) i[5] << 32))));
            o[0] = (uint32_t) r;
            o[1] = (uint32_t) (r >> 32);
        }
        break;
    case LEAF_W_LDSATOM:
        if (tid == 0) {
            acc[0] = 0;
            acc[1] = (int) 0x80000000u;
            accf[0] = 0.0f;
        }
        __syncthreads();
        lh_lds_add(&acc[0], (int) i[0]);
        lh_lds_max(&acc[1], (int) i[1]);
        lh_lds_addf(&accf[0], lh_u32_as_f32(i[2]));
        __syncthreads();
        o[0] = (uint32_t) acc[0];
        o[1] = (uint32_t) acc[1];
        o[2] = lh_f32_as_u32(accf[0]);
        break;
    default:
        break;
    }
    for (int k = 0; k < LEAF_NOUT; k++)
        out[at * LEAF_NOUT + k] = o[k];
}

/* ---- band sums: lane = band, the squares in an LDS array the host filled ---------------------------------------------
 * One array of LEAF_SQ_N floats per wave.  How far the device paths read (what LQ_SQ_AHEAD stands for in the product,
 * lh_dev_common.h): lq_band_sums_pad reads whole blocks of sixteen terms, one block ahead of the additions -- a lane
 * with n >= 1 terms reads 16 (ceil(n / 16) + 1) floats from its base, a lane with none reads nothing; lq_band_sums
 * reads 16 (ceil(maxw / 16) + 1) floats from EVERY lane's start, whatever the lane's own width.  The driver works that
 * extent out per lane and calls the leaf only if it stays inside the array for all 128 lanes (the host asserts the same
 * before it launches): otherwise nothing is read and the markers say so. */
#define LEAF_SQ_N 6144
#define LEAF_MARK_OK 0xC0DE0000u
#define LEAF_MARK_RANGE 0xBAD00000u

LH_DEVFN void
leaf_bandsum_body(int pad, const float *sq, const int *nn, const int *where, uint32_t *out)
{
    __shared__ float sqlds[2][LEAF_SQ_N] __attribute__((aligned(16)));
    __shared__ int bad[1];
    int const tid = (int) threadIdx.x, wave = tid >> 6;
    long const at = (long) blockIdx.x * LEAF_NT + tid;
    int const n = nn[at], w = where[at];        /* w: first term (pad) / first pair jj (back to back) */
    int     maxw, first, extent;
    float   r = 0.0f;
    if (tid == 0)
        bad[0] = 0;
    for (int k = tid; k < 2 * LEAF_SQ_N; k += LEAF_NT)
        (&sqlds[0][0])[k] = sq[(long) blockIdx.x * 2 * LEAF_SQ_N + k];
    __syncthreads();
    maxw = (int) lh_wave_max_u32((uint32_t) n);         /* as the product forms it (lq_zero_band_noise) */
    first = pad ? w : 2 * w;
    extent = pad ? ((n > 0) ? 16 * ((n + 15) / 16 + 1) : 0) : 16 * ((maxw + 15) / 16 + 1);
    if (n < 0 || first < 0 || first + extent > LEAF_SQ_N || (pad ? (first & 7) : 0) || (!pad && (n & 1)))
        bad[0] = 1;
    __syncthreads();
    if (lh_uni_i(bad[0]) == 0) {
        if (pad)
            r = lq_band_sums_pad(sqlds[wave], w, n, maxw);
        else
            r = lq_band_sums(sqlds[wave], n, w, maxw, n > 0);
    }
    /* every lane stores: EXEC must have come back, for the lanes without terms too */
    out[at * 4 + 0] = lh_f32_as_u32(r);
    out[at * 4 + 1] = (bad[0] ? LEAF_MARK_RANGE : LEAF_MARK_OK) | (uint32_t) tid;
    out[at * 4 + 2] = (uint32_t) maxw;
    out[at * 4 + 3] = (uint32_t) n;
}

/* ---- math leaves: one point per thread, plain loop on the CPU --------------------------------------------------------- */
enum {
    LEAF_M_POWF = 0, LEAF_M_LOGF, LEAF_M_LOG10F, LEAF_M_ADJUST, LEAF_M_MASKLOWER, LEAF_M_FASTLOG2, LEAF_M_FASTLOG2_VIA,
    LEAF_M_MASK_NEAR, LEAF_M_MASK_FAR, LEAF_M_NS_INTERP, LEAF_M_LDEXP, LEAF_M_NOPS
};

struct LeafMathArgs {
    const uint32_t *a, *b, *c;  /* inputs (b, c: where the leaf has more than one) */
    uint32_t *out;
    const float *logt;          /* LhTables.log_table, 513 floats */
    const double *mid;          /* LhTables.mask_mid, 10 doubles */
    long    n;
    int     op, flag;           /* flag: short block (lh_vbrold_adjust) */
};

LH_DEVFN uint32_t
leaf_math_eval(const LeafMathArgs & g, long k, const float *logt_lds, const double (&mid)[10])
{
    float const x = lh_u32_as_f32(g.a[k]);
    float   r = 0.0f;
#define LEAF_LOGT(m) (logt_lds[(m)])
    switch (g.op) {
    case LEAF_M_POWF:
        r = lh_powf(x, lh_u32_as_f32(g.b[k]));
        break;
    case LEAF_M_LOGF:
        r = lh_logf(x);
        break;
    case LEAF_M_LOG10F:
        r = lh_log10f(x);
        break;
    case LEAF_M_ADJUST:
        r = lh_vbrold_adjust(x, g.flag);
        break;
    case LEAF_M_MASKLOWER:
        r = lh_vbrold_masking_lower(x);
        break;
    case LEAF_M_FASTLOG2:
        r = lh_fast_log2(g.logt, x);
        break;
    case LEAF_M_FASTLOG2_VIA:
        LH_FAST_LOG2_VIA(LEAF_LOGT, x, r);
        break;
    case LEAF_M_MASK_NEAR:
        r = lh_mask_add_near(mid, x, lh_u32_as_f32(g.b[k]));
        break;
    case LEAF_M_MASK_FAR:
        r = lh_mask_add_far(x, lh_u32_as_f32(g.b[k]), mid[9]);
        break;
    case LEAF_M_NS_INTERP:
        r = lh_ns_interp(x, lh_u32_as_f32(g.b[k]), lh_u32_as_f32(g.c[k]));
        break;
    case LEAF_M_LDEXP:
        r = lq_ldexp(x, (int) g.b[k]);  /* (the host keeps the exponent the same over every 64 points: wave-uniform) */
        break;
    default:
        break;
    }
#undef LEAF_LOGT
    return lh_f32_as_u32(r);
}

#ifdef LH_EMU
/* ================================================================== CPU build */
extern "C" int
lh_leaf_wave(int op, int ncase, const uint32_t *in, uint32_t *out)
{
    if (op < 0 || op >= LEAF_W_NOPS || ncase < 1)
        return -1;
    hipemu_run(hipemu_dim3 { (unsigned) ncase, 1, 1 }, hipemu_dim3 { LEAF_NT, 1, 1 }, [=] () { leaf_wave_body(op, in, out); });
    return 0;
}

extern "C" int
lh_leaf_bandsum(int pad, int ncase, const float *sq, const int *n, const int *where, uint32_t *out)
{
    if (ncase < 1)
        return -1;
    hipemu_run(hipemu_dim3 { (unsigned) ncase, 1, 1 }, hipemu_dim3 { LEAF_NT, 1, 1 }, [=] () { leaf_bandsum_body(pad, sq, n, where, out); });
    return 0;
}

extern "C" int
lh_leaf_math(int op, long n, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, const float *logt,
             const double *midp, int flag)
{
    LeafMathArgs const g = { a, b, c, out, logt, midp, n, op, flag };
    static float tab[513];
    double  mid[10];
    if (op < 0 || op >= LEAF_M_NOPS || n < 0)
        return -1;
    for (int j = 0; j < 513; j++)
        tab[j] = logt ? logt[j] : 0.0f;
    for (int j = 0; j < 10; j++)
        mid[j] = midp ? midp[j] : 0.0;
    for (long k = 0; k < n; k++)
        out[k] = leaf_math_eval(g, k, tab, mid);
    return 0;
}

#else
/* ================================================================== device build */
extern "C" __global__ void __launch_bounds__(LEAF_NT)
lh_leaf_wave_kernel(int op, const uint32_t *in, uint32_t *out)
{
    leaf_wave_body(op, in, out);
}

extern "C" __global__ void __launch_bounds__(LEAF_NT)
lh_leaf_bandsum_kernel(int pad, const float *sq, const int *n, const int *where, uint32_t *out)
{
    leaf_bandsum_body(pad, sq, n, where, out);
}

extern "C" __global__ void __launch_bounds__(LEAF_NT)
lh_leaf_math_kernel(LeafMathArgs g)
{
    __shared__ float tab[513];
    double  mid[10];
    for (int j = (int) threadIdx.x; j < 513; j += LEAF_NT)
        tab[j] = g.logt ? g.logt[j] : 0.0f;
#pragma unroll
    for (int j = 0; j < 10; j++)
        mid[j] = g.mid ? lh_uni_f64(g.mid[j]) : 0.0;    /* wave-uniform, as lh_compute_masking holds them */
    __syncthreads();
    for (long k = (long) blockIdx.x * LEAF_NT + threadIdx.x; k < g.n; k += (long) gridDim.x * LEAF_NT)
        g.out[k] = leaf_math_eval(g, k, tab, mid);
}

/* before a launch: an error that an earlier HIP call of this thread left behind (another library's probing, say) is not
 * this launch's */
static void
leaf_begin(void)
{
    (void) hipGetLastError();
}

/* 0, or minus the HIP error of the launch, or minus (LEAF_ERR_SYNC + the HIP error of the wait for the kernel) */
#define LEAF_ERR_SYNC 10000
static int
leaf_finish(void)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return -(int) e;
    e = hipDeviceSynchronize();
    return e == hipSuccess ? 0 : -(LEAF_ERR_SYNC + (int) e);
}

/* device memory for the drivers' arrays, from the runtime this library launches with: 0 or minus the HIP error */
extern "C" int
lh_leaf_alloc(void **p, size_t bytes)
{
    hipError_t const e = hipMalloc(p, bytes ? bytes : 4);
    return e == hipSuccess ? 0 : -(int) e;
}

extern "C" int
lh_leaf_free(void *p)
{
    hipError_t const e = hipFree(p);
    return e == hipSuccess ? 0 : -(int) e;
}

extern "C" int
lh_leaf_copy(void *dst, const void *src, size_t bytes, int to_device)
{
    hipError_t const e = hipMemcpy(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : -(int) e;
}

extern "C" int
lh_leaf_wave(int op, int ncase, const uint32_t *in, uint32_t *out)
{
    if (op < 0 || op >= LEAF_W_NOPS || ncase < 1)
        return -(int) hipErrorInvalidValue;
    leaf_begin();
    hipLaunchKernelGGL(lh_leaf_wave_kernel, dim3((unsigned) ncase), dim3(LEAF_NT), 0, (hipStream_t) 0, op, in, out);
    return leaf_finish();
}

extern "C" int
lh_leaf_bandsum(int pad, int ncase, const float *sq, const int *n, const int *where, uint32_t *out)
{
    if (ncase < 1)
        return -(int) hipErrorInvalidValue;
    leaf_begin();
    hipLaunchKernelGGL(lh_leaf_bandsum_kernel, dim3((unsigned) ncase), dim3(LEAF_NT), 0, (hipStream_t) 0, pad, sq, n, where, out);
    return leaf_finish();
}

extern "C" int
lh_leaf_math(int op, long n, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, const float *logt,
             const double *midp, int flag)
{
    LeafMathArgs const g = { a, b, c, out, logt, midp, n, op, flag };
    long const blocks = (n + LEAF_NT - 1) / LEAF_NT;
    if (op < 0 || op >= LEAF_M_NOPS || n < 1)
        return -(int) hipErrorInvalidValue;
    leaf_begin();
    hipLaunchKernelGGL(lh_leaf_math_kernel, dim3((unsigned) (blocks < 8192 ? blocks : 8192)), dim3(LEAF_NT), 0, (hipStream_t) 0, g);
    return leaf_finish();
}
#endif

extern "C" int
lh_leaf_sq_n(void)
{
    return LEAF_SQ_N;
}
