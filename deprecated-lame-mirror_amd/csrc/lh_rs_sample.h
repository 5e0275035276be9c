/*
 * lh_rs_sample.h -- the per-sample arithmetic of the rate converter, ONE text for the host (lh_resample.c,
 * plain C) and the device (lh_resample_dev.hip), and the records of a conversion plan both sides read.
 *
 * Every precision step is fixed by the floats that have to come out (lh_resample.c, head comment): which
 * sub-expression is float and which double, the int -> float conversions, the order of every sum.  No
 * product may be fused with the sum that takes it: the host objects are built with -ffp-contract=off, and
 * the device text names the rounding of every product and sum as well (LH_RS_DEVICE).
 */
#ifndef LH_RS_SAMPLE_H
#define LH_RS_SAMPLE_H

#include <math.h>

#ifndef LH_RS_FN
#define LH_RS_FN static inline
#endif

#if defined(LH_RS_DEVICE) && defined(__HIP_DEVICE_COMPILE__)
#define LH_RS_FMUL(a, b) __fmul_rn((a), (b))
#define LH_RS_FADD(a, b) __fadd_rn((a), (b))
#define LH_RS_DMUL(a, b) __dmul_rn((a), (b))
#define LH_RS_DSUB(a, b) __dsub_rn((a), (b))
#else
#define LH_RS_FMUL(a, b) ((a) * (b))
#define LH_RS_FADD(a, b) ((a) + (b))
#define LH_RS_DMUL(a, b) ((a) * (b))
#define LH_RS_DSUB(a, b) ((a) - (b))
#endif

/* One block of a conversion plan (lh_rs_plan): `made' output samples from out_at on, located on the stream's
 * input -- zeros before position 0 and from the stream's length on -- with position 0 of the block at in_at. */
typedef struct LhRsBlock {
    long long in_at;
    long long out_at;
    double  start;              /* input time at which the block starts (the converter's clock) */
    int     len;                /* input samples the block had at hand */
    int     made;
} LhRsBlock;

/* A stream of a device conversion (lh_resample_dev.hip): its blocks are trunk[0 .. ntrunk) followed by
 * tail[tail_at .. tail_at + ntail). */
typedef struct LhRsStream {
    long long n;                /* input samples: nothing at or beyond is ever read */
    int     stream;             /* row pair of the pools */
    int     ntrunk;
    int     tail_at;
    int     ntail;
} LhRsStream;

/* A tile of an incremental conversion (lh_rs_block_tiles; lh_resample_dev.hip: lh_resample_tiles_kernel): outputs
 * [k0, k0 + count) of the block that starts at clock `start' with its position 0 at in_at go to out_at on (the block's
 * out_at + k0).  A tile is cut so that the input its outputs touch fits LH_RS_SPAN_MAX; lh_rs_locate counts from the
 * block's start, so a block cut into tiles gives the floats of the block done whole.  cls: the tile's rate class, an index
 * into the class table of lh_resample_mixed_tiles_kernel (a batch whose streams arrive at rates of their own); the
 * single-rate kernel never reads it.  A tile of a class that is not converted (LhRsClass.identity) is its whole block:
 * k0 = 0, outputs [out_at, out_at + count) are inputs [in_at, in_at + count) behind the PCM matrix. */
typedef struct LhRsTile {
    long long in_at;
    long long out_at;
    double  start;
    int     k0;
    int     count;
    int     stream;             /* row pair of the pools, and the entry of the launch's table of input lengths */
    int     cls;
} LhRsTile;

/* A rate class of a mixed conversion: what lh_rs_locate needs, and where the class's bank of kernels starts in the one
 * allocation that holds all banks (in floats, a multiple of 4: rows of LH_RS_ROW floats on 16-byte boundaries).
 * identity: the class's rate is the output rate, as far as the reference cares (lh_rs_needed): no bank. */
typedef struct LhRsClass {
    double  ratio;
    int     taps;
    int     phases;
    int     identity;
    long long bank_at;
} LhRsClass;

#define LH_RS_CLASSES_MAX 16   /* distinct input rates alive in one batch */

#define LH_RS_ROW 36           /* floats per kernel of the device's bank in HBM: rows start on 16-byte boundaries */
/* input positions a block's outputs can touch: its len <= 1152 samples and the taps + 1 <= 33 before them */
#define LH_RS_SPAN_MAX 1216

/* the PCM matrix in front of the converter (lame_encode_buffer's scale / scale_left / scale_right and the
 * mono downmix): l = xl m00 + xr m01, r = xl m10 + xr m11 */
typedef struct LhRsMatrix {
    float   m00, m01, m10, m11;
} LhRsMatrix;

/* what a device conversion needs besides its plan */
typedef struct LhRsParams {
    double  ratio;
    LhRsMatrix m;
    int     taps, phases;
    int     channels;
    int     one_plane;          /* mono without a downmix: the second input plane mirrors the first and is never read */
    long long cap_in, cap_out;  /* row lengths of the s16 pool and of the float pool */
} LhRsParams;

LH_RS_FN LhRsMatrix
lh_rs_matrix(float pcm_scale, float pcm_mix, float pcm_scale_r)
{
    LhRsMatrix m;
    m.m00 = pcm_scale;
    m.m01 = pcm_mix;
    m.m10 = LH_RS_FMUL(0.0f, pcm_scale);
    m.m11 = pcm_scale_r;
    return m;
}

LH_RS_FN float
lh_rs_mix(float xl, float xr, float a, float b)
{
    return LH_RS_FADD(LH_RS_FMUL(xl, a), LH_RS_FMUL(xr, b));
}

/* where output sample k of a block sits: first input position of its span and the kernel of the bank */
typedef struct LhRsSpot {
    int     first;              /* position of tap 0, from the block's position 0 */
    int     kernel;
} LhRsSpot;

LH_RS_FN LhRsSpot
lh_rs_locate(double ratio, int taps, int phases, double start, int k)
{
    LhRsSpot s;
    double const due = LH_RS_DMUL((double) k, ratio);   /* input time of the output sample, from the block's start */
    double const rel = LH_RS_DSUB(due, start);
    int const whole = (int) floor(rel);
    float const frac = (float) LH_RS_DSUB(rel, (whole + .5 * (taps % 2)));
    float const pf = (float) phases;
    /* (frac * 2 * phases) + phases in float, the trailing + .5 in double */
    float const at = LH_RS_FADD(LH_RS_FMUL(LH_RS_FMUL(frac, 2.0f), pf), pf);
    s.first = whole - taps / 2;
    s.kernel = (int) floor((double) at + .5);
    return s;
}

/* dot product of a span of taps + 1 samples with one kernel, in tap order */
LH_RS_FN float
lh_rs_dot(const float *x, const float *tap, int taps)
{
    float   acc = 0.f;
    int     i;
    for (i = 0; i <= taps; ++i)
        acc = LH_RS_FADD(acc, LH_RS_FMUL(x[i], tap[i]));
    return acc;
}

#endif
