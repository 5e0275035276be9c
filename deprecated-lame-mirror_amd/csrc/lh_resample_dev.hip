/*
 * lh_resample_dev.hip -- the rate converter of a batch on the device (gfx950): fills the batch's float pool
 * from its input pool -- s16, or the int32 / float pool of a typed batch (lh_pcm_in.h: the type's norm is part of
 * the matrix) --, bit for bit what lh_rs_block (lh_resample.c) makes of the same samples.
 *
 * The converter's serial part -- which blocks there are, and the clock each starts at -- is a plan the host
 * makes from the stream lengths alone (lh_rs_plan_tail / lh_rs_trunk_extend).  Given its block an output
 * sample depends on nothing but the stream's input: one workgroup per (stream, block) stages the span of input
 * the block's outputs touch, behind the PCM matrix and as float, in LDS -- zeros for positions before the
 * stream and from its length on, which are never read from memory --, then every lane locates its outputs
 * (lh_rs_locate) and takes the ordered dot products (lh_rs_sample.h: the host's own text) for both channels.
 * The located kernel is looked up once for the two channels.
 *
 * The bank of kernels is read through the vector cache, rows of LH_RS_ROW floats fetched 16 bytes at a time (a
 * copy of the bank in LDS, loaded once per workgroup for a run of blocks, measured 2.5 times slower: DESIGN.md).
 *
 * An incremental batch converts round by round with lh_resample_tiles_kernel, and one whose streams arrive at rates of
 * their own with lh_resample_mixed_tiles_kernel (both further down, with their own notes).
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

#define LH_RS_NT 256

struct alignas(16) LhRsF4 {
    float   v[4];
};

template < int TAPS, typename T > LH_RS_FN void
rs_convert_block(const LhRsParams & p, const float *bank, const LhRsBlock & blk, long long n,
                 const T * in_l, const T * in_r, float *out_l, float *out_r, float (*xs)[LH_RS_SPAN_MAX])
{
    int const tid = (int) threadIdx.x;
    if (blk.made <= 0)
        return;
    /* the span of input the block touches, from the first tap of its first output to the last of its last */
    int const lo = lh_rs_locate(p.ratio, TAPS, p.phases, blk.start, 0).first;
    int const count = lh_rs_locate(p.ratio, TAPS, p.phases, blk.start, blk.made - 1).first + TAPS + 1 - lo;
    if (count > LH_RS_SPAN_MAX)
        return;                 /* (no plan of the host's has such a block: lamehip_batch_set_length refuses it) */
    for (int t = tid; t < count; t += LH_RS_NT) {
        long long const at = blk.in_at + lo + t;
        float   xl = 0.0f, xr = 0.0f;
        if (at >= 0 && at < n) {
            float const sl = (float) in_l[at], sr = p.one_plane ? sl : (float) in_r[at];
            xl = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
            xr = lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
        }
        xs[0][t] = xl;
        xs[1][t] = xr;
    }
    __syncthreads();
    for (int k = tid; k < blk.made; k += LH_RS_NT) {
        LhRsSpot const s = lh_rs_locate(p.ratio, TAPS, p.phases, blk.start, k);
        const float *x0 = xs[0] + (s.first - lo), *x1 = xs[1] + (s.first - lo);
        float   a0 = 0.f, a1 = 0.f;
        const LhRsF4 *row = (const LhRsF4 *) (bank + (size_t) s.kernel * LH_RS_ROW);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            LhRsF4 const w = row[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a0 = LH_RS_FADD(a0, LH_RS_FMUL(x0[4 * q + j], w.v[j]));
                a1 = LH_RS_FADD(a1, LH_RS_FMUL(x1[4 * q + j], w.v[j]));
            }
        }
        if (TAPS == 32) {
            float const w = bank[(size_t) s.kernel * LH_RS_ROW + 32];
            a0 = LH_RS_FADD(a0, LH_RS_FMUL(x0[32], w));
            a1 = LH_RS_FADD(a1, LH_RS_FMUL(x1[32], w));
        }
        out_l[blk.out_at + k] = a0;
        out_r[blk.out_at + k] = p.channels == 1 ? 0.0f : a1;
    }
}

/* grid: x = block of the stream, y = entry of `streams' */
template < int TAPS, typename T >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_RS_NT)
#else
void
#endif
lh_resample_kernel(LhRsParams p, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails, const LhRsStream * streams,
                   const T * pcm, float *pcmf)
{
    __shared__ float xs[2][LH_RS_SPAN_MAX];
    LhRsStream const sd = streams[blockIdx.y];
    int const j = (int) blockIdx.x;
    if (j >= sd.ntrunk + sd.ntail)
        return;
    LhRsBlock const blk = j < sd.ntrunk ? trunk[j] : tails[sd.tail_at + (j - sd.ntrunk)];
    const T *in_l = pcm + (size_t) sd.stream * 2 * (size_t) p.cap_in, *in_r = in_l + p.cap_in;
    float  *out_l = pcmf + (size_t) sd.stream * 2 * (size_t) p.cap_out, *out_r = out_l + p.cap_out;
    rs_convert_block < TAPS, T > (p, bank, blk, sd.n, in_l, in_r, out_l, out_r, xs);
}

/* ---- lh_resample_tiles_kernel: the converter of an incremental batch (lamehip_batch_set_incremental_resampling) ----
 * A stream fed call by call is cut into blocks where the calls fall (lh_rs_plan_call), and a block of such a stream may
 * touch more input than LDS holds for one: the work is a TILE (LhRsTile), a run of a block's outputs whose input span the
 * host has measured to fit.  One workgroup per tile of a flat table for the whole round -- a round is ragged, most streams
 * bring a few tiles and some none --, the stream's input length from a table indexed by the tile's stream.  Staging and the
 * sums are those of rs_convert_block; the outputs are located from the BLOCK's start (k0 + k), which is what makes the
 * tiles of a block give the block's floats.
 * rs_convert_tile is one tile, the text of both tile kernels: `ratio', `phases' and `bank' are the tile's converter -- the
 * batch's here, its class's in lh_resample_mixed_tiles_kernel --, the rest of p is the batch's. */
template < int TAPS, typename T > LH_RS_FN void
rs_convert_tile(const LhRsParams & p, double ratio, int phases, const float *bank, const LhRsTile & tl, const long long *lens,
                const T * pcm, float *pcmf, float (*xs)[LH_RS_SPAN_MAX])
{
    int const tid = (int) threadIdx.x;
    /* nothing at or beyond the stream's length is read, nor beyond its row whatever the table says */
    long long const n = lens[tl.stream] < p.cap_in ? lens[tl.stream] : p.cap_in;
    const T *in_l = pcm + (size_t) tl.stream * 2 * (size_t) p.cap_in, *in_r = in_l + p.cap_in;
    float  *out_l = pcmf + (size_t) tl.stream * 2 * (size_t) p.cap_out, *out_r = out_l + p.cap_out;
    /* the span of input the tile touches, from the first tap of its first output to the last of its last */
    int const lo = lh_rs_locate(ratio, TAPS, phases, tl.start, tl.k0).first;
    int const span = lh_rs_locate(ratio, TAPS, phases, tl.start, tl.k0 + tl.count - 1).first + TAPS + 1 - lo;
    if (span > LH_RS_SPAN_MAX || tl.out_at < 0 || tl.out_at + tl.count > p.cap_out)
        return;                 /* (no tile of the host's is such: lh_rs_block_tiles, and the appends' capacity check) */
    for (int t = tid; t < span; t += LH_RS_NT) {
        long long const at = tl.in_at + lo + t;
        float   xl = 0.0f, xr = 0.0f;
        if (at >= 0 && at < n) {
            float const sl = (float) in_l[at], sr = p.one_plane ? sl : (float) in_r[at];
            xl = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
            xr = lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
        }
        xs[0][t] = xl;
        xs[1][t] = xr;
    }
    __syncthreads();
    for (int k = tid; k < tl.count; k += LH_RS_NT) {
        LhRsSpot const s = lh_rs_locate(ratio, TAPS, phases, tl.start, tl.k0 + k);
        const float *x0 = xs[0] + (s.first - lo), *x1 = xs[1] + (s.first - lo);
        float   a0 = 0.f, a1 = 0.f;
        const LhRsF4 *row = (const LhRsF4 *) (bank + (size_t) s.kernel * LH_RS_ROW);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            LhRsF4 const w = row[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a0 = LH_RS_FADD(a0, LH_RS_FMUL(x0[4 * q + j], w.v[j]));
                a1 = LH_RS_FADD(a1, LH_RS_FMUL(x1[4 * q + j], w.v[j]));
            }
        }
        if (TAPS == 32) {
            float const w = bank[(size_t) s.kernel * LH_RS_ROW + 32];
            a0 = LH_RS_FADD(a0, LH_RS_FMUL(x0[32], w));
            a1 = LH_RS_FADD(a1, LH_RS_FMUL(x1[32], w));
        }
        out_l[tl.out_at + k] = a0;
        out_r[tl.out_at + k] = p.channels == 1 ? 0.0f : a1;
    }
}

template < int TAPS, typename T >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_RS_NT)
#else
void
#endif
lh_resample_tiles_kernel(LhRsParams p, const float *bank, const LhRsTile * tiles, const long long *lens, const T * pcm, float *pcmf)
{
    __shared__ float xs[2][LH_RS_SPAN_MAX];
    LhRsTile const tl = tiles[blockIdx.x];
    if (tl.count <= 0)
        return;
    rs_convert_tile < TAPS, T > (p, p.ratio, p.phases, bank, tl, lens, pcm, pcmf, xs);
}

/* ---- lh_resample_mixed_tiles_kernel: the same round for a batch whose streams arrive at rates of their own ----
 * (lamehip_batch_set_stream_in_samplerate).  Every tile names its rate class (LhRsTile.cls), and a table of classes in HBM
 * says what lh_rs_locate needs for it and where its bank starts in the one allocation that holds all banks: ONE launch
 * converts a round at any mix of ratios.  Tile and class record are the same for every lane of the workgroup -- scalar
 * loads, and a uniform branch to the 31- or 32-tap body, which is rs_convert_tile's, the single-rate kernel's own text.
 * A class that is not converted (identity: the reference passes such a rate through, lh_rs_needed) copies: outputs
 * [out_at, out_at + count) are inputs [in_at + k0, ...) behind the PCM matrix -- what lh_append_kernel would have
 * written --, zeros from the stream's length on (the flush), no LDS, nothing outside the tile's samples read.  p.ratio,
 * p.taps and p.phases are not looked at. */
template < typename T >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_RS_NT)
#else
void
#endif
lh_resample_mixed_tiles_kernel(LhRsParams p, const LhRsClass * classes, int nclasses, const float *banks, const LhRsTile * tiles,
                               const long long *lens, const T * pcm, float *pcmf)
{
    __shared__ float xs[2][LH_RS_SPAN_MAX];
    LhRsTile const tl = tiles[blockIdx.x];
    if (tl.count <= 0 || tl.cls < 0 || tl.cls >= nclasses)
        return;
    LhRsClass const c = classes[tl.cls];
    if (c.identity) {
        long long const n = lens[tl.stream] < p.cap_in ? lens[tl.stream] : p.cap_in;
        const T *in_l = pcm + (size_t) tl.stream * 2 * (size_t) p.cap_in, *in_r = in_l + p.cap_in;
        float  *out_l = pcmf + (size_t) tl.stream * 2 * (size_t) p.cap_out, *out_r = out_l + p.cap_out;
        if (tl.k0 < 0 || tl.in_at < 0 || tl.out_at < 0 || tl.out_at + tl.count > p.cap_out)
            return;
        for (int k = (int) threadIdx.x; k < tl.count; k += LH_RS_NT) {
            long long const at = tl.in_at + tl.k0 + k;
            float   xl = 0.0f, xr = 0.0f;
            if (at < n) {
                float const sl = (float) in_l[at], sr = p.one_plane ? sl : (float) in_r[at];
                xl = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
                xr = lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
            }
            out_l[tl.out_at + k] = xl;
            out_r[tl.out_at + k] = p.channels == 1 ? 0.0f : xr;
        }
        return;
    }
    if (c.phases < 1 || c.phases > 320 || c.bank_at < 0)
        return;
    if (c.taps == 31)
        rs_convert_tile < 31, T > (p, c.ratio, c.phases, banks + c.bank_at, tl, lens, pcm, pcmf, xs);
    else if (c.taps == 32)
        rs_convert_tile < 32, T > (p, c.ratio, c.phases, banks + c.bank_at, tl, lens, pcm, pcmf, xs);
}

#ifndef LH_EMU
template < typename T > static int
rs_launch_mixed(const LhRsParams * p, const LhRsClass * classes, int nclasses, const float *banks, const LhRsTile * tiles, long long ntiles,
                const long long *lens, const T * pcm, float *pcmf, void *stream)
{
    if (ntiles <= 0)
        return 0;
    if (nclasses < 1 || nclasses > LH_RS_CLASSES_MAX || ntiles > 0x7fffffffLL)
        return (int) hipErrorInvalidValue;
    hipLaunchKernelGGL((lh_resample_mixed_tiles_kernel < T >), dim3((unsigned) ntiles), dim3(LH_RS_NT), 0, (hipStream_t) stream, *p, classes,
                       nclasses, banks, tiles, lens, pcm, pcmf);
    return (int) hipGetLastError();
}

/* lh_launch_resample_tiles for a round of mixed rates: `classes' (device) holds nclasses records, every tile's cls an
 * index into it, every record's bank_at an offset into `banks' (device).  Returns a hipError_t. */
extern "C" int
lh_launch_resample_mixed_tiles(int type, const LhRsParams * p, const LhRsClass * classes, int nclasses, const float *banks,
                               const LhRsTile * tiles, long long ntiles, const long long *lens, const void *pcm, float *pcmf, void *stream)
{
    switch (type) {
    case LH_PCM_S16:
        return rs_launch_mixed(p, classes, nclasses, banks, tiles, ntiles, lens, (const int16_t *) pcm, pcmf, stream);
    case LH_PCM_S32:
        return rs_launch_mixed(p, classes, nclasses, banks, tiles, ntiles, lens, (const int32_t *) pcm, pcmf, stream);
    case LH_PCM_F32:
    case LH_PCM_F32_UNIT:
        return rs_launch_mixed(p, classes, nclasses, banks, tiles, ntiles, lens, (const float *) pcm, pcmf, stream);
    }
    return (int) hipErrorInvalidValue;
}

template < typename T > static int
rs_launch_tiles(const LhRsParams * p, const float *bank, const LhRsTile * tiles, long long ntiles, const long long *lens, const T * pcm,
                float *pcmf, void *stream)
{
    if (ntiles <= 0)
        return 0;
    if ((p->taps != 31 && p->taps != 32) || p->phases < 1 || p->phases > 320 || ntiles > 0x7fffffffLL)
        return (int) hipErrorInvalidValue;
    dim3 const grid((unsigned) ntiles), block(LH_RS_NT);
    if (p->taps == 31)
        hipLaunchKernelGGL((lh_resample_tiles_kernel < 31, T >), grid, block, 0, (hipStream_t) stream, *p, bank, tiles, lens, pcm, pcmf);
    else
        hipLaunchKernelGGL((lh_resample_tiles_kernel < 32, T >), grid, block, 0, (hipStream_t) stream, *p, bank, tiles, lens, pcm, pcmf);
    return (int) hipGetLastError();
}

/* ntiles entries of `tiles' (device), every tile's stream an index into `lens' (device: input samples per stream); `pcm' is
 * a pool of `type' (LH_PCM_*), whose norm the caller has put into p->m (lh_pcm_matrix; lh_rs_matrix for s16).  The caller
 * has checked every tile against the float pool's rows.  Returns a hipError_t. */
extern "C" int
lh_launch_resample_tiles(int type, const LhRsParams * p, const float *bank, const LhRsTile * tiles, long long ntiles,
                         const long long *lens, const void *pcm, float *pcmf, void *stream)
{
    switch (type) {
    case LH_PCM_S16:
        return rs_launch_tiles(p, bank, tiles, ntiles, lens, (const int16_t *) pcm, pcmf, stream);
    case LH_PCM_S32:
        return rs_launch_tiles(p, bank, tiles, ntiles, lens, (const int32_t *) pcm, pcmf, stream);
    case LH_PCM_F32:
    case LH_PCM_F32_UNIT:
        return rs_launch_tiles(p, bank, tiles, ntiles, lens, (const float *) pcm, pcmf, stream);
    }
    return (int) hipErrorInvalidValue;
}

template < typename T > static int
rs_launch(const LhRsParams * p, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails, const LhRsStream * streams,
          int nstreams, int max_blocks, const T * pcm, float *pcmf, void *stream)
{
    if (nstreams <= 0 || max_blocks <= 0)
        return 0;
    if ((p->taps != 31 && p->taps != 32) || p->phases < 1 || p->phases > 320)
        return (int) hipErrorInvalidValue;
    /* (blockIdx.y ends at 65535: a longer list goes in slices) */
    for (int at = 0; at < nstreams; at += 65535) {
        int const ns = nstreams - at < 65535 ? nstreams - at : 65535;
        dim3 const grid((unsigned) max_blocks, (unsigned) ns), block(LH_RS_NT);
        if (p->taps == 31)
            hipLaunchKernelGGL((lh_resample_kernel < 31, T >), grid, block, 0, (hipStream_t) stream, *p, bank, trunk, tails, streams + at,
                               pcm, pcmf);
        else
            hipLaunchKernelGGL((lh_resample_kernel < 32, T >), grid, block, 0, (hipStream_t) stream, *p, bank, trunk, tails, streams + at,
                               pcm, pcmf);
        hipError_t const e = hipGetLastError();
        if (e != hipSuccess)
            return (int) e;
    }
    return 0;
}

/* nstreams entries of `streams', the longest with max_blocks blocks; `pcm' is a pool of `type' (LH_PCM_*), whose norm
 * the caller has put into p->m (lh_pcm_matrix).  Returns a hipError_t. */
extern "C" int
lh_launch_resample_typed(int type, const LhRsParams * p, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails,
                         const LhRsStream * streams, int nstreams, int max_blocks, const void *pcm, float *pcmf, void *stream)
{
    switch (type) {
    case LH_PCM_S16:
        return rs_launch(p, bank, trunk, tails, streams, nstreams, max_blocks, (const int16_t *) pcm, pcmf, stream);
    case LH_PCM_S32:
        return rs_launch(p, bank, trunk, tails, streams, nstreams, max_blocks, (const int32_t *) pcm, pcmf, stream);
    case LH_PCM_F32:
    case LH_PCM_F32_UNIT:
        return rs_launch(p, bank, trunk, tails, streams, nstreams, max_blocks, (const float *) pcm, pcmf, stream);
    }
    return (int) hipErrorInvalidValue;
}

/* the s16 case */
extern "C" int
lh_launch_resample(const LhRsParams * p, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails,
                   const LhRsStream * streams, int nstreams, int max_blocks, const int16_t * pcm, float *pcmf, void *stream)
{
    return rs_launch(p, bank, trunk, tails, streams, nstreams, max_blocks, pcm, pcmf, stream);
}
#else
template < typename T > static int
rs_emu(const LhRsParams * params, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails, const LhRsStream * streams,
       int nstreams, int max_blocks, const T * pcm, float *pcmf)
{
    LhRsParams const p = *params;
    hipemu_dim3 grid = { (unsigned) max_blocks, (unsigned) nstreams, 1 }, block = { LH_RS_NT, 1, 1 };
    if (nstreams <= 0 || max_blocks <= 0)
        return 0;
    hipemu_run(grid, block,[=] () {
               if (p.taps == 31)
                   lh_resample_kernel < 31, T > (p, bank, trunk, tails, streams, pcm, pcmf);
               else
                   lh_resample_kernel < 32, T > (p, bank, trunk, tails, streams, pcm, pcmf);
               }
    );
    return 0;
}

extern "C" int
lh_emu_resample_typed(int type, const LhRsParams * params, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails,
                      const LhRsStream * streams, int nstreams, int max_blocks, const void *pcm, float *pcmf)
{
    switch (type) {
    case LH_PCM_S16:
        return rs_emu(params, bank, trunk, tails, streams, nstreams, max_blocks, (const int16_t *) pcm, pcmf);
    case LH_PCM_S32:
        return rs_emu(params, bank, trunk, tails, streams, nstreams, max_blocks, (const int32_t *) pcm, pcmf);
    case LH_PCM_F32:
    case LH_PCM_F32_UNIT:
        return rs_emu(params, bank, trunk, tails, streams, nstreams, max_blocks, (const float *) pcm, pcmf);
    }
    return -1;
}

template < typename T > static int
rs_emu_tiles(const LhRsParams * params, const float *bank, const LhRsTile * tiles, long long ntiles, const long long *lens, const T * pcm,
             float *pcmf)
{
    LhRsParams const p = *params;
    hipemu_dim3 grid = { (unsigned) ntiles, 1, 1 }, block = { LH_RS_NT, 1, 1 };
    if (ntiles <= 0)
        return 0;
    hipemu_run(grid, block,[=] () {
               if (p.taps == 31)
                   lh_resample_tiles_kernel < 31, T > (p, bank, tiles, lens, pcm, pcmf);
               else
                   lh_resample_tiles_kernel < 32, T > (p, bank, tiles, lens, pcm, pcmf);
               }
    );
    return 0;
}

extern "C" int
lh_emu_resample_tiles(int type, const LhRsParams * params, const float *bank, const LhRsTile * tiles, long long ntiles,
                      const long long *lens, const void *pcm, float *pcmf)
{
    switch (type) {
    case LH_PCM_S16:
        return rs_emu_tiles(params, bank, tiles, ntiles, lens, (const int16_t *) pcm, pcmf);
    case LH_PCM_S32:
        return rs_emu_tiles(params, bank, tiles, ntiles, lens, (const int32_t *) pcm, pcmf);
    case LH_PCM_F32:
    case LH_PCM_F32_UNIT:
        return rs_emu_tiles(params, bank, tiles, ntiles, lens, (const float *) pcm, pcmf);
    }
    return -1;
}

template < typename T > static int
rs_emu_mixed(const LhRsParams * params, const LhRsClass * classes, int nclasses, const float *banks, const LhRsTile * tiles, long long ntiles,
             const long long *lens, const T * pcm, float *pcmf)
{
    LhRsParams const p = *params;
    hipemu_dim3 grid = { (unsigned) ntiles, 1, 1 }, block = { LH_RS_NT, 1, 1 };
    if (ntiles <= 0)
        return 0;
    hipemu_run(grid, block,[=] () {
               lh_resample_mixed_tiles_kernel < T > (p, classes, nclasses, banks, tiles, lens, pcm, pcmf);
               }
    );
    return 0;
}

extern "C" int
lh_emu_resample_mixed_tiles(int type, const LhRsParams * params, const LhRsClass * classes, int nclasses, const float *banks,
                            const LhRsTile * tiles, long long ntiles, const long long *lens, const void *pcm, float *pcmf)
{
    switch (type) {
    case LH_PCM_S16:
        return rs_emu_mixed(params, classes, nclasses, banks, tiles, ntiles, lens, (const int16_t *) pcm, pcmf);
    case LH_PCM_S32:
        return rs_emu_mixed(params, classes, nclasses, banks, tiles, ntiles, lens, (const int32_t *) pcm, pcmf);
    case LH_PCM_F32:
    case LH_PCM_F32_UNIT:
        return rs_emu_mixed(params, classes, nclasses, banks, tiles, ntiles, lens, (const float *) pcm, pcmf);
    }
    return -1;
}

extern "C" int
lh_emu_resample(const LhRsParams * params, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails,
                const LhRsStream * streams, int nstreams, int max_blocks, const int16_t * pcm, float *pcmf)
{
    return rs_emu(params, bank, trunk, tails, streams, nstreams, max_blocks, pcm, pcmf);
}
#endif
