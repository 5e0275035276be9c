/*
 * lh_ingest.hip -- the front door of a typed batch on the device (gfx950): lh_ingest_kernel fills the batch's float
 * pool from its int32 / float input pool, bit for bit what lh_pcm_ingest_host (lh_pcm_in.c) makes of the same
 * samples -- lame_copy_inbuffer's arithmetic (lh_pcm_in.h) --, lh_deinterleave_kernel takes an interleaved
 * device buffer apart into two rows of the input pool (lamehip_batch_set_input_device with stride 2), and
 * lh_append_kernel (further down, with its own notes) puts the chunks of an incremental batch at their places.
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

/* ---- lh_append_kernel: the front door of an incremental batch (lamehip_batch_append_input / _append_device) ----
 * A table of segments (LhApSeg, lh_pcm_in.h), each a chunk of one stream in the batch's element type -- in the staging
 * arena or in the caller's own device buffers, planar or interleaved -- goes to its place in the pool the kernels read:
 * an int32 / float chunk through lh_rs_mix into the float pool, what lh_ingest_kernel would have written at the same
 * positions; an s16 chunk as it is into the s16 pool (the front kernels apply the matrix, as for lamehip_batch_append);
 * and a chunk of a batch that converts the rate round by round as it is into the INPUT pool, whatever its type (4-byte
 * elements as uint32_t: the converter applies matrix and norm, lh_resample_dev.hip).
 *
 * The same stream as the ingest, in UNITS of 16 destination bytes (four floats, eight shorts).  A segment's `at' moves
 * the destination's alignment independently of the row's, so p0 -- the first position at which the left destination
 * starts a unit -- is the segment's own; how the sources lie there is decided once per workgroup: a planar source that
 * is aligned as well is loaded a unit at a time, an interleaved one (r = l + 1) a pair at a time -- one load of two
 * elements yields both planes, 16 bytes at a time where the pairs are aligned to that --, anything else element by
 * element.  The at most G - 1 positions before p0 and behind the last whole unit are done one by one by the segment's
 * first workgroup.  The grid is sized by the launch's longest segment: a workgroup beyond its own segment's end leaves
 * at once.  No LDS, no cross-lane traffic. */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(LH_EMU)
#define LH_AP_GLOBAL __attribute__((address_space(1)))
#else
#define LH_AP_GLOBAL
#endif
template < typename E, int N, int A > struct alignas(A) LhApVec {
    E       v[N];
};

/* N consecutive elements behind p, which is aligned to 16 bytes (level 2), to two elements (1) or to one (0) */
template < typename E, int N > LH_RS_FN LhApVec < E, N, sizeof(E) > ap_load(const E * p, int level)
{
    LhApVec < E, N, sizeof(E) > r;
    if (level == 2) {
        LhApVec < E, N, 16 > const q = *(const LhApVec < E, N, 16 > *)p;
#pragma unroll
        for (int j = 0; j < N; ++j)
            r.v[j] = q.v[j];
    }
    else if (level == 1) {
        LhApVec < E, N, 2 * sizeof(E) > const q = *(const LhApVec < E, N, 2 * sizeof(E) > *)p;
#pragma unroll
        for (int j = 0; j < N; ++j)
            r.v[j] = q.v[j];
    }
    else
        r = *(const LhApVec < E, N, sizeof(E) > *)p;
    return r;
}

template < typename D, int N > LH_RS_FN void
ap_store(D * p, bool aligned, const LhApVec < D, N, sizeof(D) > &r)
{
    if (aligned) {
        LhApVec < D, N, 16 > q;
#pragma unroll
        for (int j = 0; j < N; ++j)
            q.v[j] = r.v[j];
        *(LhApVec < D, N, 16 > *)p = q;
    }
    else
        *(LhApVec < D, N, sizeof(D) > *)p = r;
}

LH_RS_FN int
ap_level(const void *p, size_t pair)
{
    return ((uintptr_t) p & 15) == 0 ? 2 : ((uintptr_t) p & (pair - 1)) == 0 ? 1 : 0;
}

/* what the pool holds for a sample of type T: the float lame_copy_inbuffer makes of it, or the short itself */
template < typename T > struct LhApDst {
    typedef float type;
};
template <> struct LhApDst <int16_t > {
    typedef int16_t type;
};
/* (uint32_t: a 4-byte element as it is -- the int32 / float input pool of a batch that converts the rate round by round,
 * whose converter applies the matrix and the type's norm; bits are moved, nothing is computed) */
template <> struct LhApDst <uint32_t > {
    typedef uint32_t type;
};

LH_RS_FN void
ap_put(int16_t xl, int16_t xr, const LhInParams & p, int16_t * u, int16_t * v)
{
    (void) p;
    *u = xl;
    *v = xr;
}

LH_RS_FN void
ap_put(uint32_t xl, uint32_t xr, const LhInParams & p, uint32_t * u, uint32_t * v)
{
    (void) p;
    *u = xl;
    *v = xr;
}

template < typename T > LH_RS_FN void
ap_put(T xl, T xr, const LhInParams & p, float *u, float *v)
{
    float const sl = (float) xl, sr = (float) xr;
    *u = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
    *v = p.channels == 1 ? 0.0f : lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
}

/* grid: x = LH_IN_QUADS units of the segment, y = entry of `segs' */
template < typename T >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_IN_NT)
#else
void
#endif
lh_append_kernel(LhInParams p, const LhApSeg * segs, void *pool)
{
    typedef typename LhApDst < T >::type D;
    constexpr int G = 16 / (int) sizeof(D);
    LhApSeg const sd = segs[blockIdx.y];
    int const tid = (int) threadIdx.x;
    long long const n = sd.n, q0 = (long long) blockIdx.x * LH_IN_QUADS;
    /* (uniform: the launch's grid is the longest segment's) */
    if (n <= 0 || (blockIdx.x != 0 && q0 * G >= n))
        return;
    D      *out_l = (D *) pool + ((size_t) sd.stream * 2 * (size_t) p.cap + (size_t) sd.at), *out_r = out_l + p.cap;
    /* (addresses from a table: said to be global memory, or every load through them would be a flat one) */
    const T *in_l = (const T *) (LH_AP_GLOBAL const T *) (uintptr_t) sd.l, *in_r = (const T *) (LH_AP_GLOBAL const T *) (uintptr_t) sd.r;
    bool const one_plane = p.one_plane != 0;
    long long const st = sd.stride;
    /* first position at which the left destination starts a 16-byte unit, and the whole units from there on */
    int const p0 = (int) (((16 - ((uintptr_t) out_l & 15)) & 15) / sizeof(D));
    long long const full = n > p0 ? (n - p0) / G : 0;
    bool const al_or = in_aligned16(out_r + p0);
    /* interleaved with both planes wanted: a pair per load.  (One plane: the elements between the left samples are not
     * the caller's to be read, the last of them may lie beyond the buffer.) */
    bool const pairs = st == 2 && !one_plane && in_r == in_l + 1;
    int const lv_l = pairs ? ap_level(in_l + 2 * p0, 2 * sizeof(T)) : in_aligned16(in_l + p0) ? 2 : 0;
    int const lv_r = in_aligned16(in_r + p0) ? 2 : 0;
#pragma unroll
    for (int step = 0; step < LH_IN_STEPS; ++step) {
        long long const q = q0 + step * LH_IN_NT + tid;
        if (q < full) {
            long long const at = p0 + G * q;    /* at + G - 1 <= p0 + G full - 1 < n */
            LhApVec < T, G, sizeof(T) > xl, xr;
            if (pairs) {
                LhApVec < T, 2 * G, sizeof(T) > const x = ap_load < T, 2 * G > (in_l + 2 * at, lv_l);
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    xl.v[j] = x.v[2 * j];
                    xr.v[j] = x.v[2 * j + 1];
                }
            }
            else if (st == 1) {
                xl = ap_load < T, G > (in_l + at, lv_l);
                xr = one_plane ? xl : ap_load < T, G > (in_r + at, lv_r);
            }
            else {
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    xl.v[j] = in_l[st * (at + j)];
                    xr.v[j] = one_plane ? xl.v[j] : in_r[st * (at + j)];
                }
            }
            LhApVec < D, G, sizeof(D) > u, v;
#pragma unroll
            for (int j = 0; j < G; ++j)
                ap_put(xl.v[j], xr.v[j], p, &u.v[j], &v.v[j]);
            ap_store < D, G > (out_l + at, true, u);
            ap_store < D, G > (out_r + at, al_or, v);
        }
    }
    /* the edges, one position per lane: [0, p0) and [p0 + G full, n) */
    if (blockIdx.x == 0 && tid < 2 * (G - 1)) {
        long long const at = tid < G - 1 ? tid : p0 + G * full + (tid - (G - 1));
        if (at < n && (tid >= G - 1 || at < p0)) {
            T const xl = in_l[st * at], xr = one_plane ? xl : in_r[st * at];
            ap_put(xl, xr, p, &out_l[at], &out_r[at]);
        }
    }
}

/* workgroups along x for segments of at most max_n samples, `unit' of them to 16 destination bytes */
static unsigned
append_blocks(long long max_n, int unit)
{
    long long const k = (max_n / unit + LH_IN_QUADS - 1) / LH_IN_QUADS;
    return (unsigned) (k > 0 ? k : 1);
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

/* nsegs entries of `segs' (device), the longest of max_n samples, into `pool': the s16 pool for LH_PCM_S16 (p->m is not
 * used), else the float pool.  The caller has checked every segment against the rows (at + n <= p->cap).  Returns a
 * hipError_t. */
extern "C" int
lh_launch_append(int type, const LhInParams * p, const LhApSeg * segs, int nsegs, long long max_n, void *pool, void *stream)
{
    if (nsegs <= 0 || max_n <= 0)
        return 0;
    if (type < 0 || type >= LH_PCM_TYPES || max_n > p->cap)
        return (int) hipErrorInvalidValue;
    /* (blockIdx.y ends at 65535: a longer list goes in slices) */
    for (int at = 0; at < nsegs; at += 65535) {
        int const ns = nsegs - at < 65535 ? nsegs - at : 65535;
        dim3 const grid(append_blocks(max_n, type == LH_PCM_S16 ? 8 : 4), (unsigned) ns), block(LH_IN_NT);
        if (type == LH_PCM_S16)
            hipLaunchKernelGGL((lh_append_kernel < int16_t >), grid, block, 0, (hipStream_t) stream, *p, segs + at, pool);
        else if (type == LH_PCM_S32)
            hipLaunchKernelGGL((lh_append_kernel < int32_t >), grid, block, 0, (hipStream_t) stream, *p, segs + at, pool);
        else
            hipLaunchKernelGGL((lh_append_kernel < float >), grid, block, 0, (hipStream_t) stream, *p, segs + at, pool);
        hipError_t const e = hipGetLastError();
        if (e != hipSuccess)
            return (int) e;
    }
    return 0;
}

/* the same into an INPUT pool of elements of esz bytes (2 or 4), every sample as it is: p->m and p->channels are not used,
 * p->cap is the input pool's row length.  Returns a hipError_t. */
extern "C" int
lh_launch_append_raw(int esz, const LhInParams * p, const LhApSeg * segs, int nsegs, long long max_n, void *pool, void *stream)
{
    if (nsegs <= 0 || max_n <= 0)
        return 0;
    if ((esz != 2 && esz != 4) || max_n > p->cap)
        return (int) hipErrorInvalidValue;
    for (int at = 0; at < nsegs; at += 65535) {
        int const ns = nsegs - at < 65535 ? nsegs - at : 65535;
        dim3 const grid(append_blocks(max_n, 16 / esz), (unsigned) ns), block(LH_IN_NT);
        if (esz == 2)
            hipLaunchKernelGGL((lh_append_kernel < int16_t >), grid, block, 0, (hipStream_t) stream, *p, segs + at, pool);
        else
            hipLaunchKernelGGL((lh_append_kernel < uint32_t >), grid, block, 0, (hipStream_t) stream, *p, segs + at, pool);
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
lh_emu_append(int type, const LhInParams * params, const LhApSeg * segs, int nsegs, long long max_n, void *pool)
{
    LhInParams const p = *params;
    hipemu_dim3 grid = { append_blocks(max_n, type == LH_PCM_S16 ? 8 : 4), (unsigned) nsegs, 1 }, block = { LH_IN_NT, 1, 1 };
    if (nsegs <= 0 || max_n <= 0)
        return 0;
    if (type < 0 || type >= LH_PCM_TYPES || max_n > p.cap)
        return -1;
    hipemu_run(grid, block,[=] () {
               if (type == LH_PCM_S16)
                   lh_append_kernel < int16_t > (p, segs, pool);
               else if (type == LH_PCM_S32)
                   lh_append_kernel < int32_t > (p, segs, pool);
               else
                   lh_append_kernel < float >(p, segs, pool);
               }
    );
    return 0;
}

extern "C" int
lh_emu_append_raw(int esz, const LhInParams * params, const LhApSeg * segs, int nsegs, long long max_n, void *pool)
{
    LhInParams const p = *params;
    hipemu_dim3 grid = { append_blocks(max_n, esz == 2 ? 8 : 4), (unsigned) nsegs, 1 }, block = { LH_IN_NT, 1, 1 };
    if (nsegs <= 0 || max_n <= 0)
        return 0;
    if ((esz != 2 && esz != 4) || max_n > p.cap)
        return -1;
    hipemu_run(grid, block,[=] () {
               if (esz == 2)
                   lh_append_kernel < int16_t > (p, segs, pool);
               else
                   lh_append_kernel < uint32_t > (p, segs, pool);
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
