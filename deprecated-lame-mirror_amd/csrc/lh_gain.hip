/*
 * lh_gain.hip -- the radio gain of a batch's streams on the device (gfx950): lh_gain_kernel passes every stream
 * through the two equal-loudness filters and adds up the squares of every 50 ms window, bit for bit what lh_rg_block
 * (lh_replaygain.c) makes of the same samples handed over in the same blocks.  What comes out is the list of window
 * sums (lsum, rsum) per stream; the truncated log10 that turns a sum into a histogram bin stays on the host
 * (lh_rg_bin), so that no bin depends on a device log10.
 *
 * The filters' feedback is rounded to float at every sample, so a (stream, channel) is one serial chain; a wave takes
 * one stream and keeps everything else off that chain.  LH_GN_RUN samples at a time -- one per lane --:
 *   A  the samples are loaded (behind the PCM matrix where the pool is s16; zeros from the stream's length on, which
 *      are generated, never read) into a ring of the last 128 in LDS;
 *   B  the first filter's feed-forward sum, eleven taps, per lane;
 *   C  its feedback, sample after sample, in one of two mappings (template parameter TAPS; lh_batch.cpp chooses by the
 *      launch's size, LH_GN_TAPS_BELOW): the ten taps across the lanes of a 16-lane row, rows 0 and 1 the channels, products
 *      in parallel and the ordered double sum walking up the row through DPP moves -- or all ten taps in registers of
 *      lanes 0 (left) and 1 (right);
 *   D  the second filter's feed-forward sum per lane, E its feedback in lanes 0 and 1;
 *   F  per lane: where the sample sits in its piece -- pieces are cut as lh_rg_block cuts them: at a block's start,
 *      ten samples into it, and at a window's end -- and with that the term it closes: the square of a head sample
 *      (n mod 4 of them, double products) or a sum of four float squares;
 *   G  lanes 0 and 1 add the terms up in order: into the piece's sum, that into the window's, and store a finished
 *      window.
 * The blocks come from the host's plan (lh_gain.h): the wave walks them as it goes.  Only wave-level synchronisation;
 * the LH_GN_WAVES waves of a workgroup share nothing.
 * Every rounding is named (lh_gain.h).  Built with -ffp-contract=off like every object of the library, and without
 * flushing subnormals: the first filter's output is subnormal within a thousand samples of silence and stays so.
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
#include "lh_wave.h"
#include "lh_gain.h"

#define LH_GN_NT (64 * LH_GN_WAVES)
#define LH_GN_RING (2 * LH_GN_RUN)

/* a wave's LDS: the last LH_GN_RING samples before, between and behind the filters, and a double per sample of the run */
struct LhGainLds {
    float   x[2][LH_GN_RING], mid[2][LH_GN_RING], out[2][LH_GN_RING];
    double  d[2][LH_GN_RUN];
};

#define GN_AT(ring, pos, back) ((ring)[((pos) - (back)) & (LH_GN_RING - 1)])

/* length of block j of a stream */
LH_RS_FN int
gain_block_len(const LhGainStream & sd, int fs, const int *trunk, const int *tails, int j)
{
    if (j < sd.ntrunk)
        return trunk ? trunk[j] : fs;
    return tails[sd.tail_at + (j - sd.ntrunk)];
}

/* feed-forward sum of the first filter at `pos' (piece_energy's s1) */
LH_RS_FN double
gain_yule_forward(const float *x, int pos, const float *ky)
{
    double const y0 = LH_GN_TAP(GN_AT(x, pos, 10), ky[0]), y2 = LH_GN_TAP(GN_AT(x, pos, 9), ky[1]);
    double const y4 = LH_GN_TAP(GN_AT(x, pos, 8), ky[2]), y6 = LH_GN_TAP(GN_AT(x, pos, 7), ky[3]);
    double const s00 = LH_GN_DADD(LH_GN_DADD(LH_GN_DADD(y0, y2), y4), y6);
    double const y8 = LH_GN_TAP(GN_AT(x, pos, 6), ky[4]), yA = LH_GN_TAP(GN_AT(x, pos, 5), ky[5]);
    double const yC = LH_GN_TAP(GN_AT(x, pos, 4), ky[6]), yE = LH_GN_TAP(GN_AT(x, pos, 3), ky[7]);
    double const s01 = LH_GN_DADD(LH_GN_DADD(LH_GN_DADD(y8, yA), yC), yE);
    double const yG = LH_GN_TAP2(GN_AT(x, pos, 2), ky[8], GN_AT(x, pos, 1), ky[9]);
    double const yK = LH_GN_TAP(GN_AT(x, pos, 0), ky[10]);
    return LH_GN_DADD(LH_GN_DADD(LH_GN_DADD(s00, s01), yG), yK);
}

/* feedback sum of the first filter (piece_energy's s2): q[j] is the output j + 1 samples back */
LH_RS_FN double
gain_yule_feedback(const float (&q)[LH_GN_ORDER], const float *ky)
{
    double const x1 = LH_GN_TAP2(q[9], ky[11], q[8], ky[12]);
    double const x5 = LH_GN_TAP2(q[7], ky[13], q[6], ky[14]);
    double const x9 = LH_GN_TAP2(q[5], ky[15], q[4], ky[16]);
    double const xD = LH_GN_TAP2(q[3], ky[17], q[2], ky[18]);
    double const xH = LH_GN_TAP2(q[1], ky[19], q[0], ky[20]);
    return LH_GN_DADD(LH_GN_DADD(LH_GN_DADD(LH_GN_DADD(x1, x5), x9), xD), xH);
}

/* grid: x = LH_GN_WAVES entries of `streams' */
template < typename T, int TAPS >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_GN_NT)
#else
void
#endif
lh_gain_kernel(LhGainParams p, const LhGainStream * streams, int nstreams, const int *trunk, const int *tails, const T * pool,
               double *pairs)
{
    __shared__ LhGainLds lds[LH_GN_WAVES];
    int const lane = lh_lane(), wave = lh_wave_id();
    int const si = (int) blockIdx.x * LH_GN_WAVES + wave;
    if (si >= nstreams)
        return;                 /* (the whole wave: nothing below waits for another wave) */
    LhGainLds & L = lds[wave];
    LhGainStream const sd = streams[si];
    int const nch = p.channels == 1 ? 1 : 2, W = p.window;
    int const nblk = sd.ntrunk + sd.ntail;
    const T *row_l = pool + (size_t) sd.stream * 2 * (size_t) p.cap, *row_r = row_l + p.cap;
    double *out = pairs + 2 * sd.win_at;
    /* what lanes 0 and 1 carry from run to run: the filters' histories and the sums; every lane: the block cursor */
    float   q[LH_GN_ORDER], o1 = 0.0f, o2 = 0.0f;
    double  sum = 0.0, wsum = 0.0;
    int     wins = 0;
    int     blk = 0, blk_at = 0, blk_len = nblk > 0 ? gain_block_len(sd, p.fs, trunk, tails, 0) : 0;
    /* TAPS: lane r < 10 of a row of 16 holds the first filter's output 10 - r samples back and its feedback tap; rows 0 and 1
     * are the channels (rows 2 and 3 shadow them and store nothing) */
    int const tap = lane & 15, tap_ch = (lane >> 4) & 1;
    bool const tap_writer = tap == 8 && (lane >> 4) < nch;
    float   kt = 0.0f, h = 0.0f;
#pragma unroll
    for (int j = 0; j < LH_GN_ORDER; ++j) {
        q[j] = 0.0f;
        if (tap == j)
            kt = p.ky[11 + j];
    }
    for (int c = 0; c < 2; ++c)
        for (int k = lane; k < LH_GN_RING; k += 64)
            L.x[c][k] = L.mid[c][k] = L.out[c][k] = 0.0f;
    LH_WAVE_SYNC();
    for (int at = 0; at < sd.total; at += LH_GN_RUN) {
        int const pos = at + lane, slot = pos & (LH_GN_RING - 1), half = at & LH_GN_RUN;
        /* A */
        {
            float   xl = 0.0f, xr = 0.0f;
            if (pos < sd.n) {
                if (sizeof(T) == 2) {
                    float const sl = (float) row_l[pos], sr = p.one_plane ? sl : (float) row_r[pos];
                    xl = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
                    if (nch == 2)
                        xr = lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
                }
                else {
                    xl = (float) row_l[pos];
                    if (nch == 2)
                        xr = (float) row_r[pos];
                }
            }
            L.x[0][slot] = xl;
            L.x[1][slot] = xr;
        }
        LH_WAVE_SYNC();
        /* B */
        for (int c = 0; c < nch; ++c)
            L.d[c][lane] = gain_yule_forward(L.x[c], pos, p.ky);
        LH_WAVE_SYNC();
        /* C */
        if (TAPS) {
            /* one instruction stream for both channels: the ten products at once, the pairs (float sums) on the even lanes,
             * then the ordered double sum walks up the row two lanes at a time -- x1 in lane 0, + x5 in lane 2, + x9, + xD,
             * + xH in lane 8, which forms the output; the history moves down a lane and takes the output in at lane 9 */
            const double *s1 = L.d[tap_ch];
            float  *mid = L.mid[tap_ch] + half;
#pragma unroll 8
            for (int i = 0; i < LH_GN_RUN; ++i) {
                float const pr = LH_GN_FMUL(h, kt);
                double const x = (double) LH_GN_FADD(pr, lh_row_shl_f32 < 1 > (pr));
                double  acc = x;
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                float const v = LH_GN_NARROW(LH_GN_DSUB(s1[i], acc));
                if (tap_writer)
                    mid[i] = v;
                float const older = lh_row_shl_f32 < 1 > (h), newest = lh_row_shr_f32 < 1 > (v);
                h = tap == 9 ? newest : older;
            }
        }
        else if (lane < nch) {
            const double *s1 = L.d[lane];
            float  *mid = L.mid[lane] + half;
            for (int i0 = 0; i0 < LH_GN_RUN; i0 += 16) {
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    float const v = LH_GN_NARROW(LH_GN_DSUB(s1[i0 + u], gain_yule_feedback(q, p.ky)));
#pragma unroll
                    for (int j = LH_GN_ORDER - 1; j > 0; --j)
                        q[j] = q[j - 1];
                    q[0] = v;
                    mid[i0 + u] = v;
                }
            }
        }
        LH_WAVE_SYNC();
        /* D */
        for (int c = 0; c < nch; ++c) {
            const float *m = L.mid[c];
            /* (three products in one float expression) */
            L.d[c][lane] = (double) LH_GN_FADD(LH_GN_FADD(LH_GN_FMUL(GN_AT(m, pos, 2), p.kb[0]), LH_GN_FMUL(GN_AT(m, pos, 1), p.kb[2])),
                                               LH_GN_FMUL(GN_AT(m, pos, 0), p.kb[4]));
        }
        LH_WAVE_SYNC();
        /* E */
        if (lane < nch) {
            const double *s1 = L.d[lane];
            float  *o = L.out[lane] + half;
#pragma unroll 16
            for (int i = 0; i < LH_GN_RUN; ++i) {
                double const s2 = LH_GN_TAP2(o2, p.kb[1], o1, p.kb[3]);
                float const v = LH_GN_NARROW(LH_GN_DSUB(s1[i], s2));
                o2 = o1;
                o1 = v;
                o[i] = v;
            }
        }
        LH_WAVE_SYNC();
        /* F */
        bool const valid = pos < sd.total;
        int     j = blk, b0 = blk_at, bn = blk_len;
        while (valid && pos >= b0 + bn && j + 1 < nblk) {
            b0 += bn;
            ++j;
            bn = gain_block_len(sd, p.fs, trunk, tails, j);
        }
        int const w0 = (pos / W) * W, in_blk = pos - b0;
        int     first = b0 + (in_blk >= LH_GN_ORDER ? LH_GN_ORDER : 0), end = b0 + bn;
        if (w0 > first)
            first = w0;
        if (in_blk < LH_GN_ORDER && b0 + LH_GN_ORDER < end)
            end = b0 + LH_GN_ORDER;
        if (w0 + W < end)
            end = w0 + W;
        int const k = pos - first, head = (end - first) & 3;
        bool const single = valid && k < head, four = valid && k >= head && ((k - head) & 3) == 3;
        for (int c = 0; c < nch; ++c) {
            const float *o = L.out[c];
            double  t = 0.0;
            if (single) {
                double const v = (double) GN_AT(o, pos, 0);
                t = LH_GN_DMUL(v, v);
            }
            else if (four) {
                float const fa = GN_AT(o, pos, 3), fb = GN_AT(o, pos, 2), fc = GN_AT(o, pos, 1), fd = GN_AT(o, pos, 0);
                t = LH_GN_DADD(LH_GN_DADD(LH_GN_DADD(LH_GN_TAP(fa, fa), LH_GN_TAP(fb, fb)), LH_GN_TAP(fc, fc)), LH_GN_TAP(fd, fd));
            }
            L.d[c][lane] = t;
        }
        uint64_t const m_term = lh_ballot(single || four), m_last = lh_ballot(valid && pos == end - 1);
        uint64_t const m_win = lh_ballot(valid && pos == w0 + W - 1);
        LH_WAVE_SYNC();
        /* G */
        if (lane < nch) {
            uint64_t m = m_term | m_last;
            while (m) {
                int const i = lh_ffs64(m);
                m &= m - 1;
                if ((m_term >> i) & 1)
                    sum = LH_GN_DADD(sum, L.d[lane][i]);
                if ((m_last >> i) & 1) {
                    wsum = LH_GN_DADD(wsum, sum);
                    sum = 0.0;
                    if ((m_win >> i) & 1) {
                        out[2 * (long long) wins + lane] = wsum;
                        if (nch == 1)
                            out[2 * (long long) wins + 1] = wsum;
                        wsum = 0.0;
                        ++wins;
                    }
                }
            }
        }
        blk = (int) lh_bcast_u32((uint32_t) j, 63);
        blk_at = (int) lh_bcast_u32((uint32_t) b0, 63);
        blk_len = (int) lh_bcast_u32((uint32_t) bn, 63);
        LH_WAVE_SYNC();
    }
}

#ifndef LH_EMU
/* nstreams entries of `streams' (device), `pool' s16 or -- floats != 0 -- float.  Returns a hipError_t. */
extern "C" int
lh_launch_gain(int floats, const LhGainParams * p, const LhGainStream * streams, int nstreams, const int *trunk, const int *tails,
               const void *pool, double *pairs, void *stream)
{
    if (nstreams <= 0)
        return 0;
    if (p->window < 1 || p->fs < 1)
        return (int) hipErrorInvalidValue;
    dim3 const grid((unsigned) ((nstreams + LH_GN_WAVES - 1) / LH_GN_WAVES)), block(LH_GN_NT);
#define GN_LAUNCH(T, TAPS) hipLaunchKernelGGL((lh_gain_kernel < T, TAPS >), grid, block, 0, (hipStream_t) stream, *p, streams, \
                                             nstreams, trunk, tails, (const T *) pool, pairs)
    if (floats && p->taps)
        GN_LAUNCH(float, 1);
    else if (floats)
        GN_LAUNCH(float, 0);
    else if (p->taps)
        GN_LAUNCH(int16_t, 1);
    else
        GN_LAUNCH(int16_t, 0);
    return (int) hipGetLastError();
}
#else
extern "C" int
lh_emu_gain(int floats, const LhGainParams * params, const LhGainStream * streams, int nstreams, const int *trunk, const int *tails,
            const void *pool, double *pairs)
{
    LhGainParams const p = *params;
    hipemu_dim3 grid = { (unsigned) ((nstreams + LH_GN_WAVES - 1) / LH_GN_WAVES), 1, 1 }, block = { LH_GN_NT, 1, 1 };
    if (nstreams <= 0)
        return 0;
    if (p.window < 1 || p.fs < 1)
        return -1;
    hipemu_run(grid, block,[=] () {
               if (floats && p.taps)
                   lh_gain_kernel < float, 1 > (p, streams, nstreams, trunk, tails, (const float *) pool, pairs);
               else if (floats)
                   lh_gain_kernel < float, 0 > (p, streams, nstreams, trunk, tails, (const float *) pool, pairs);
               else if (p.taps)
                   lh_gain_kernel < int16_t, 1 > (p, streams, nstreams, trunk, tails, (const int16_t *) pool, pairs);
               else
                   lh_gain_kernel < int16_t, 0 > (p, streams, nstreams, trunk, tails, (const int16_t *) pool, pairs);
               }
    );
    return 0;
}
#endif
