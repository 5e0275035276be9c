/*
 * lh_ingest.hip -- the front door of a typed batch on the device (gfx950): lh_ingest_kernel fills the batch's float
 * pool from its int32 / float input pool, bit for bit what lh_pcm_ingest_host (lh_pcm_in.c) makes of the same
 * samples -- lame_copy_inbuffer's arithmetic (lh_pcm_in.h) --, and lh_deinterleave_kernel takes an interleaved
 * device buffer apart into two rows of the input pool (lamehip_batch_set_input_device with stride 2).
 *
 * The ingest is a pure stream: 4 bytes in and 4 bytes out per sample and plane.  A lane takes QUADS: four
 * consecutive positions of both planes (u and v each need xl and xr), loaded and stored 16 bytes at a time.  The
 * pools' row length is the caller's, so a row starts on a 16-byte boundary only for some residues of
 * (stream * 2 + ch) * capacity: the quads start at the first position p0 at which the left float row does, which of
 * the other three rows are aligned there as well is decided once per workgroup (uniform branches; a row that is not
 * goes through 4-byte-aligned accesses), and the positions before p0 and behind the last whole quad -- at most three
 * each -- are done one by one by the stream's first workgroup.  Nothing at or beyond a stream's length is read or
 * written.  No LDS, no cross-lane traffic.
 * Built with -ffp-contract=off like every object of the library.
 */
#include <stdint.h>
#include <math.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_RS_FN static inline
#else
#include <hip/hip_runtime.h>
#define LH_RS_DEVICE
#define LH_RS_FN static __device__ __forceinline__
#endif
#include "lh_pcm_in.h"

/* four consecutive elements of a row, behind a pointer aligned to A bytes */
template < typename E, int A > struct alignas(A) LhInQuad {
    E       v[4];
};

template < typename E > LH_RS_FN LhInQuad < E, 4 > in_load4(const E * p, bool aligned)
{
    LhInQuad < E, 4 > r;
    if (aligned) {
        LhInQuad < E, 16 > const q = *(const LhInQuad < E, 16 > *)p;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            r.v[j] = q.v[j];
    }
    else
        r = *(const LhInQuad < E, 4 > *)p;
    return r;
}

LH_RS_FN void
in_store4(float *p, bool aligned, const LhInQuad < float, 4 > &r)
{
    if (aligned) {
        LhInQuad < float, 16 > q;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            q.v[j] = r.v[j];
        *(LhInQuad < float, 16 > *)p = q;
    }
    else
        *(LhInQuad < float, 4 > *)p = r;
}

LH_RS_FN bool
in_aligned16(const void *p)
{
    return ((uintptr_t) p & 15) == 0;
}

/* grid: x = LH_IN_QUADS quads of the stream, y = entry of `streams' */
template < typename T >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_IN_NT)
#else
void
#endif
lh_ingest_kernel(LhInParams p, const LhInStream * streams, const T * in, float *out)
{
    LhInStream const sd = streams[blockIdx.y];
    int const tid = (int) threadIdx.x;
    long long const n = sd.n < p.cap ? sd.n : p.cap;
    const T *in_l = in + (size_t) sd.stream * 2 * (size_t) p.cap, *in_r = in_l + p.cap;
    float  *out_l = out + (size_t) sd.stream * 2 * (size_t) p.cap, *out_r = out_l + p.cap;
    bool const one_plane = p.one_plane != 0, mono = p.channels == 1;
    /* first position at which the left float row starts a 16-byte unit, and the whole quads from there on */
    int const p0 = (int) (((16 - ((uintptr_t) out_l & 15)) & 15) >> 2);
    long long const full = n > p0 ? (n - p0) / 4 : 0;
    bool const al_il = in_aligned16(in_l + p0), al_ir = in_aligned16(in_r + p0), al_or = in_aligned16(out_r + p0);
    long long const q0 = (long long) blockIdx.x * LH_IN_QUADS;
#pragma unroll
    for (int step = 0; step < LH_IN_STEPS; ++step) {
        long long const q = q0 + step * LH_IN_NT + tid;
        if (q < full) {
            long long const at = p0 + 4 * q;    /* at + 3 <= p0 + 4 full - 1 < n */
            LhInQuad < T, 4 > const xl = in_load4(in_l + at, al_il);
            LhInQuad < T, 4 > const xr = one_plane ? xl : in_load4(in_r + at, al_ir);
            LhInQuad < float, 4 > u, v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float const sl = (float) xl.v[j], sr = (float) xr.v[j];
                u.v[j] = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
                v.v[j] = mono ? 0.0f : lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
            }
            in_store4(out_l + at, true, u);
            in_store4(out_r + at, al_or, v);
        }
    }
    /* the edges, one position per lane: [0, p0) and [p0 + 4 full, n) */
    if (blockIdx.x == 0 && tid < 6) {
        long long const at = tid < 3 ? tid : p0 + 4 * full + (tid - 3);
        if (at < n && (tid >= 3 || at < p0)) {
            float const sl = (float) in_l[at], sr = one_plane ? sl : (float) in_r[at];
            out_l[at] = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
            out_r[at] = mono ? 0.0f : lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
        }
    }
}

/* dst_l[i] = src_l[2 i], dst_r[i] = src_r[2 i] for i < n (src_r = src_l + 1: an interleaved buffer); dst_r == NULL:
 * the left plane alone, src_r is never read.  One position per lane. */
template < typename T >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_IN_NT)
#else
void
#endif
lh_deinterleave_kernel(const T * src_l, const T * src_r, T * dst_l, T * dst_r, long long n)
{
    long long const i = (long long) blockIdx.x * LH_IN_NT + (long long) threadIdx.x;
    if (i >= n)
        return;
    dst_l[i] = src_l[2 * i];
    if (dst_r)
        dst_r[i] = src_r[2 * i];
}

/* workgroups along x for streams of at most max_n samples */
static unsigned
ingest_blocks(long long max_n)
{
    long long const k = (max_n / 4 + LH_IN_QUADS - 1) / LH_IN_QUADS;
    return (unsigned) (k > 0 ? k : 1);
}

#ifndef LH_EMU
/* nstreams entries of `streams', the longest of max_n samples; `in' is the pool of `type' (LH_PCM_S32 / _F32 /
 * _F32_UNIT: the matrix carries the type's norm).  Returns a hipError_t. */
extern "C" int
lh_launch_ingest(int type, const LhInParams * p, const LhInStream * streams, int nstreams, long long max_n, const void *in,
                 float *out, void *stream)
{
    if (nstreams <= 0 || max_n <= 0)
        return 0;
    if ((type != LH_PCM_S32 && type != LH_PCM_F32 && type != LH_PCM_F32_UNIT) || max_n > p->cap)
        return (int) hipErrorInvalidValue;
    /* (blockIdx.y ends at 65535: a longer list goes in slices) */
    for (int at = 0; at < nstreams; at += 65535) {
        int const ns = nstreams - at < 65535 ? nstreams - at : 65535;
        dim3 const grid(ingest_blocks(max_n), (unsigned) ns), block(LH_IN_NT);
        if (type == LH_PCM_S32)
            hipLaunchKernelGGL((lh_ingest_kernel < int32_t >), grid, block, 0, (hipStream_t) stream, *p, streams + at,
                               (const int32_t *) in, out);
        else
            hipLaunchKernelGGL((lh_ingest_kernel < float >), grid, block, 0, (hipStream_t) stream, *p, streams + at,
                               (const float *) in, out);
        hipError_t const e = hipGetLastError();
        if (e != hipSuccess)
            return (int) e;
    }
    return 0;
}

/* elements of esz bytes (2 or 4).  Returns a hipError_t. */
extern "C" int
lh_launch_deinterleave(int esz, const void *src_l, const void *src_r, void *dst_l, void *dst_r, long long n, void *stream)
{
    if (n <= 0)
        return 0;
    if ((esz != 2 && esz != 4) || n > (long long) 0x7fffffff * LH_IN_NT)
        return (int) hipErrorInvalidValue;
    dim3 const grid((unsigned) ((n + LH_IN_NT - 1) / LH_IN_NT)), block(LH_IN_NT);
    if (esz == 2)
        hipLaunchKernelGGL((lh_deinterleave_kernel < int16_t >), grid, block, 0, (hipStream_t) stream, (const int16_t *) src_l,
                           (const int16_t *) src_r, (int16_t *) dst_l, (int16_t *) dst_r, n);
    else
        hipLaunchKernelGGL((lh_deinterleave_kernel < int32_t >), grid, block, 0, (hipStream_t) stream, (const int32_t *) src_l,
                           (const int32_t *) src_r, (int32_t *) dst_l, (int32_t *) dst_r, n);
    return (int) hipGetLastError();
}
#else
extern "C" int
lh_emu_ingest(int type, const LhInParams * params, const LhInStream * streams, int nstreams, long long max_n, const void *in,
              float *out)
{
    LhInParams const p = *params;
    hipemu_dim3 grid = { ingest_blocks(max_n), (unsigned) nstreams, 1 }, block = { LH_IN_NT, 1, 1 };
    if (nstreams <= 0 || max_n <= 0)
        return 0;
    if ((type != LH_PCM_S32 && type != LH_PCM_F32 && type != LH_PCM_F32_UNIT) || max_n > p.cap)
        return -1;
    hipemu_run(grid, block,[=] () {
               if (type == LH_PCM_S32)
                   lh_ingest_kernel < int32_t > (p, streams, (const int32_t *) in, out);
               else
                   lh_ingest_kernel < float >(p, streams, (const float *) in, out);
               }
    );
    return 0;
}

extern "C" int
lh_emu_deinterleave(int esz, const void *src_l, const void *src_r, void *dst_l, void *dst_r, long long n)
{
    hipemu_dim3 grid = { (unsigned) ((n + LH_IN_NT - 1) / LH_IN_NT), 1, 1 }, block = { LH_IN_NT, 1, 1 };
    if (n <= 0)
        return 0;
    if (esz != 2 && esz != 4)
        return -1;
    hipemu_run(grid, block,[=] () {
               if (esz == 2)
                   lh_deinterleave_kernel < int16_t > ((const int16_t *) src_l, (const int16_t *) src_r, (int16_t *) dst_l,
                                                       (int16_t *) dst_r, n);
               else
                   lh_deinterleave_kernel < int32_t > ((const int32_t *) src_l, (const int32_t *) src_r, (int32_t *) dst_l,
                                                       (int32_t *) dst_r, n);
               }
    );
    return 0;
}
#endif
