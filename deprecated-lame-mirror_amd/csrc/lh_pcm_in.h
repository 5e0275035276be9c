/*
 * lh_pcm_in.h -- the sample types of a batch and lame_copy_inbuffer's arithmetic (reference lame.c:1786-1872),
 * ONE text for the host (lh_pcm_in.c, lh_batch.cpp) and the device (lh_ingest.hip, lh_resample_dev.hip), beside
 * lh_rs_sample.h, whose matrix record and rounding names it uses.
 *
 * A sample of any type becomes float (int32 -> float rounds to nearest even on both sides), then
 *     u = xl m00 + xr m01,  v = xl m10 + xr m11        (lh_rs_mix: every product and sum rounded to float, nothing fused)
 * with the matrix of lame_encode_buffer_template: the type's norm times { scale, mix; 0 * scale, scale_r }.
 */
#ifndef LH_PCM_IN_H
#define LH_PCM_IN_H

#include <stdint.h>
#include "lh_rs_sample.h"

/* (the values of LAMEHIP_PCM_* in include/lamehip.h) */
#define LH_PCM_S16      0       /* int16_t, +/- 32768: lame_encode_buffer */
#define LH_PCM_S32      1       /* int32_t, +/- 2^31: lame_encode_buffer_int */
#define LH_PCM_F32      2       /* float, +/- 32768: lame_encode_buffer_float */
#define LH_PCM_F32_UNIT 3       /* float, +/- 1.0: lame_encode_buffer_ieee_float */
#define LH_PCM_TYPES    4

LH_RS_FN int
lh_pcm_elem_size(int type)
{
    return type == LH_PCM_S16 ? 2 : 4;
}

/* the `norm' lame_encode_buffer_template is called with */
LH_RS_FN float
lh_pcm_norm(int type)
{
    return type == LH_PCM_S32 ? (float) (1.0 / 65536.0) : type == LH_PCM_F32_UNIT ? 32767.0f : 1.0f;
}

LH_RS_FN LhRsMatrix
lh_pcm_matrix(int type, float pcm_scale, float pcm_mix, float pcm_scale_r)
{
    float const norm = lh_pcm_norm(type);
    LhRsMatrix m;
    m.m00 = LH_RS_FMUL(norm, pcm_scale);
    m.m01 = LH_RS_FMUL(norm, pcm_mix);
    m.m10 = LH_RS_FMUL(norm, LH_RS_FMUL(0.0f, pcm_scale));
    m.m11 = LH_RS_FMUL(norm, pcm_scale_r);
    return m;
}

/* A stream of an ingest launch (lh_ingest.hip): rows `stream' of the typed pool become rows `stream' of the float pool
 * up to n; nothing at or beyond n is read or written. */
typedef struct LhInStream {
    long long n;
    int     stream;
    int     pad_;
} LhInStream;

/* what an ingest launch needs besides its list */
typedef struct LhInParams {
    LhRsMatrix m;
    int     channels;           /* 1: the second float plane gets zeros (the rate converter's convention) */
    int     one_plane;          /* mono without a downmix: the second input plane mirrors the first and is never read */
    long long cap;              /* row length of both pools */
} LhInParams;

/* A segment of an append launch (lh_ingest.hip): n samples of the batch's element type, the left ones from device
 * address l on and the right ones from r on, `stride' elements from one sample to the next (1: planar; 2: interleaved,
 * r = l + one element), go to positions [at, at + n) of rows `stream' -- of the float pool through the arithmetic above
 * when the batch's type is int32 / float, of the s16 pool as they are when it is s16.  Nothing outside the segment's
 * samples is read, nothing outside [at, at + n) is written; with one_plane set r is never read. */
typedef struct LhApSeg {
    unsigned long long l, r;
    long long at;
    long long n;
    int     stream;
    int     stride;
} LhApSeg;

#define LH_IN_NT 256            /* lanes of a workgroup */
#define LH_IN_STEPS 4           /* quads of four positions per lane */
#define LH_IN_QUADS (LH_IN_NT * LH_IN_STEPS)    /* quads per workgroup: 4096 positions of a stream */

#endif
