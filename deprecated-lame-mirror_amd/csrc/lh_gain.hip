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
 * the LH_GN_WAVES waves of a workgroup share nothing (4 KB of LDS each, 16 KB per workgroup, in either kernel).
 *
 * The kernels' text lies in lh_gain_stream.h and is compiled twice: as lh_gain_kernel (GN_RESUME 0), which the compiler
 * turns into the instructions it made of it before there was a second kernel, and as lh_gain_resume_kernel (GN_RESUME 1),
 * the same text for an incremental batch: a launch is a ROUND -- what was appended to a stream since the last round, as
 * the blocks the calls made of it -- and what a stream carries from round
 * to round lies in its LhGainCarry (lh_gain.h).  Positions are counted from the round's start, `base' = carry.heard samples
 * into the stream, so the ring's slots and the halves of mid / out (at & LH_GN_RUN) are addressed as in a whole stream
 * whatever base is: the carry's ten inputs, ten first-filter outputs and two second-filter outputs go into the ring's slots
 * for positions -10 .. -1, and both mappings of C take their history from there -- lanes 0 to 9 of rows 0 and 1, or q[] --,
 * which keeps them bit-equal to each other and lets the host choose the mapping anew every round.  Only the windows are
 * absolute: they end at multiples of W of the samples heard.
 * INVARIANT the resumed kernel relies on: a round ends at a block's end.  So no piece sum is open at a round's boundary
 * (only the window's sums are carried), a group of four squares never reaches back into the round before, and the block
 * cursor restarts at 0 with every round.  The last run's lanes beyond the round's end have run the filters on zeros: the
 * carry is therefore read back from the ring at the round's end, not from the registers, and stored with ordinary
 * stores.  The inputs are kept in the carry rather than read from the pool again: the ring holds them already, behind the
 * PCM matrix, and a float pool's rows need no second look.
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

/* the kernels' text, compiled twice (lh_gain_stream.h) */
#define GN_RESUME 0
#include "lh_gain_stream.h"
#undef GN_RESUME
#define GN_RESUME 1
#include "lh_gain_stream.h"
#undef GN_RESUME

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

/* a round of an incremental batch: nstreams entries of `streams' (device) -- total and tails the round's, ntrunk 0 --, from
 * and to `carry' (device, one record per stream of the batch).  Returns a hipError_t. */
extern "C" int
lh_launch_gain_resume(int floats, const LhGainParams * p, const LhGainStream * streams, int nstreams, const int *tails, const void *pool,
                      double *pairs, LhGainCarry * carry, void *stream)
{
    if (nstreams <= 0)
        return 0;
    if (p->window < 1 || p->fs < 1 || !carry)
        return (int) hipErrorInvalidValue;
    dim3 const grid((unsigned) ((nstreams + LH_GN_WAVES - 1) / LH_GN_WAVES)), block(LH_GN_NT);
#define GN_RESUME(T, TAPS) hipLaunchKernelGGL((lh_gain_resume_kernel < T, TAPS >), grid, block, 0, (hipStream_t) stream, *p, streams, \
                                             nstreams, tails, (const T *) pool, pairs, carry)
    if (floats && p->taps)
        GN_RESUME(float, 1);
    else if (floats)
        GN_RESUME(float, 0);
    else if (p->taps)
        GN_RESUME(int16_t, 1);
    else
        GN_RESUME(int16_t, 0);
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

extern "C" int
lh_emu_gain_resume(int floats, const LhGainParams * params, const LhGainStream * streams, int nstreams, const int *tails, const void *pool,
                   double *pairs, LhGainCarry * carry)
{
    LhGainParams const p = *params;
    hipemu_dim3 grid = { (unsigned) ((nstreams + LH_GN_WAVES - 1) / LH_GN_WAVES), 1, 1 }, block = { LH_GN_NT, 1, 1 };
    if (nstreams <= 0)
        return 0;
    if (p.window < 1 || p.fs < 1 || !carry)
        return -1;
    hipemu_run(grid, block,[=] () {
               if (floats && p.taps)
                   lh_gain_resume_kernel < float, 1 > (p, streams, nstreams, tails, (const float *) pool, pairs, carry);
               else if (floats)
                   lh_gain_resume_kernel < float, 0 > (p, streams, nstreams, tails, (const float *) pool, pairs, carry);
               else if (p.taps)
                   lh_gain_resume_kernel < int16_t, 1 > (p, streams, nstreams, tails, (const int16_t *) pool, pairs, carry);
               else
                   lh_gain_resume_kernel < int16_t, 0 > (p, streams, nstreams, tails, (const int16_t *) pool, pairs, carry);
               }
    );
    return 0;
}
#endif
