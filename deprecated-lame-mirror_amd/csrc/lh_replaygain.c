/*
 * lh_replaygain.c -- the "radio gain" of the stream that lame_encode_buffer feeds, for the LAME tag
 * (reference gain_analysis.c:199-476 + lame.c:1715-1720, 1565-1580; host C, handle API only: the frontend switches
 * it on by default, the library's own default is off).
 *
 * The measure (ReplayGain proposal): both channels pass an equal-loudness filter -- a 10th order IIR fitted to
 * the inverse loudness curve, then a 2nd order high-pass --, the mean square of every 50 ms window goes into a
 * histogram with 0.01 dB bins, and the title's level is the bin that 95 % of the windows stay below; the gain is
 * what brings that to the 89 dB reference (pink noise calibration 64.82 dB).
 *
 * Bit-exactness with the reference needs three things kept: the products of a filter tap are formed in float and
 * added in double in the reference's grouping; a window's squares are added piece by piece, where a piece is what
 * one call contributes to the window -- its first ten samples apart (the reference reads those from a prefix
 * buffer) --, inside a piece first n mod 4 single squares, then sums of four; the histogram bin is the truncated
 * double.  What is this file's own: a streaming formulation (ten samples of input / intermediate / output history
 * per channel instead of the reference's window-sized buffers that are shifted at every window end).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"
#include "lh_replaygain_tables.h"
#include "lh_gain.h"

#define RG_ORDER 10

int
lh_rg_start(LhReplayGain * g, int samplerate)
{
    static const int rates[9] = { 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000 };
    int     i;
    memset(g, 0, sizeof(*g));
    g->rate_index = -1;
    for (i = 0; i < 9; i++)
        if (rates[i] == samplerate)
            g->rate_index = i;
    if (g->rate_index < 0)
        return -1;
    g->window = (samplerate * 1L + 20L - 1) / 20L;      /* 50 ms, rounded up */
    return 0;
}

/* one piece of one channel: n samples at x (the ten before them in hist_in), through both filters; the outputs'
 * squares are added up in the reference's grouping */
static double
piece_energy(LhReplayGain * g, int ch, const float *x, int n)
{
    const float *ky = lh_rg_yule[g->rate_index], *kb = lh_rg_butter[g->rate_index];
    float  *in = g->work[0], *mid = g->work[1], *out = g->work[2];
    const float *o;
    double  sum = 0;
    int     i;
    memcpy(in, g->hist_in[ch], RG_ORDER * sizeof(float));
    memcpy(in + RG_ORDER, x, (size_t) n * sizeof(float));
    memcpy(mid, g->hist_mid[ch], RG_ORDER * sizeof(float));
    memcpy(out, g->hist_out[ch], RG_ORDER * sizeof(float));
    for (i = 0; i < n; i++) {
        const float *p = in + RG_ORDER + i;
        float  *q = mid + RG_ORDER + i;
        double const y0 = p[-10] * ky[0], y2 = p[-9] * ky[1], y4 = p[-8] * ky[2], y6 = p[-7] * ky[3];
        double const s00 = y0 + y2 + y4 + y6;
        double const y8 = p[-6] * ky[4], yA = p[-5] * ky[5], yC = p[-4] * ky[6], yE = p[-3] * ky[7];
        double const s01 = y8 + yA + yC + yE;
        double const yG = p[-2] * ky[8] + p[-1] * ky[9];
        double const yK = p[0] * ky[10];
        double const s1 = s00 + s01 + yG + yK;
        double const x1 = q[-10] * ky[11] + q[-9] * ky[12];
        double const x5 = q[-8] * ky[13] + q[-7] * ky[14];
        double const x9 = q[-6] * ky[15] + q[-5] * ky[16];
        double const xD = q[-4] * ky[17] + q[-3] * ky[18];
        double const xH = q[-2] * ky[19] + q[-1] * ky[20];
        double const s2 = x1 + x5 + x9 + xD + xH;
        q[0] = (float) (s1 - s2);
    }
    for (i = 0; i < n; i++) {
        const float *p = mid + RG_ORDER + i;
        float  *q = out + RG_ORDER + i;
        double const s1 = p[-2] * kb[0] + p[-1] * kb[2] + p[0] * kb[4];
        double const s2 = q[-2] * kb[1] + q[-1] * kb[3];
        q[0] = (float) (s1 - s2);
    }
    o = out + RG_ORDER;
    for (i = n & 3; i > 0; i--) {
        double const v = *o++;
        sum += v * v;
    }
    for (i = n / 4; i > 0; i--) {
        double const a = o[0] * o[0], b = o[1] * o[1], c = o[2] * o[2], d = o[3] * o[3];
        double const four = a + b + c + d;
        sum += four;
        o += 4;
    }
    /* the last ten of each become the history (a piece shorter than ten keeps part of the old one) */
    memcpy(g->hist_in[ch], in + n, RG_ORDER * sizeof(float));
    memcpy(g->hist_mid[ch], mid + n, RG_ORDER * sizeof(float));
    memcpy(g->hist_out[ch], out + n, RG_ORDER * sizeof(float));
    return sum;
}

/* the histogram bin of a finished window: its mean square in 0.01 dB steps, truncated (the one place a log10 is taken:
 * the batch's device analysis hands its window sums to this very text) */
size_t
lh_rg_bin(double lsum, double rsum, long window)
{
    double const level = 100 * 10. * log10((lsum + rsum) / window * 0.5 + 1.e-37);
    size_t  bin = (level <= 0) ? 0 : (size_t) level;
    if (bin >= LH_RG_BINS)
        bin = LH_RG_BINS - 1;
    return bin;
}

/* one block; with `nwin', finished windows are counted there and their sums kept in pairs[2 k], pairs[2 k + 1] for k < cap */
static int
rg_block(LhReplayGain * g, const float *l, const float *r, int n, int channels, double *pairs, long cap, long *nwin)
{
    int     at = 0;
    if (g->rate_index < 0 || n <= 0)
        return 0;
    if (n > LH_RG_MAX_BLOCK)
        return -1;
    if (channels == 1)
        r = l;
    while (at < n) {
        long    take = n - at;
        if (take > g->window - g->filled)
            take = g->window - g->filled;
        if (at < RG_ORDER && take > RG_ORDER - at)
            take = RG_ORDER - at;       /* the call's first ten samples are a piece of their own */
        g->lsum += piece_energy(g, 0, l + at, (int) take);
        g->rsum += piece_energy(g, 1, r + at, (int) take);
        at += (int) take;
        g->filled += take;
        if (g->filled == g->window) {
            g->bins[lh_rg_bin(g->lsum, g->rsum, g->filled)]++;
            if (nwin) {
                if (pairs && *nwin < cap) {
                    pairs[2 * *nwin] = g->lsum;
                    pairs[2 * *nwin + 1] = g->rsum;
                }
                ++*nwin;
            }
            g->lsum = g->rsum = 0.;
            g->filled = 0;
        }
    }
    return 0;
}

/* one block as lame_encode_buffer hands it to the analysis (at most one frame's worth of samples) */
int
lh_rg_block(LhReplayGain * g, const float *l, const float *r, int n, int channels)
{
    return rg_block(g, l, r, n, channels, NULL, 0, NULL);
}

/* the gain in tenths of a dB as the tag stores it (reference lame.c:1571-1578) that a histogram of windows stands
 * for: the bin 95 % of them stay below, against the 89 dB reference; 0 when there is no window */
int
lh_rg_tenths(const uint32_t * bins)
{
    unsigned long windows = 0, upper, seen = 0;
    size_t  i;
    float   gain;
    for (i = 0; i < LH_RG_BINS; i++)
        windows += bins[i];
    if (windows == 0)
        return 0;
    upper = (unsigned long) (uint32_t) ceil((uint32_t) windows * (1. - 0.95));
    for (i = LH_RG_BINS; i-- > 0;) {
        seen += bins[i];
        if (seen >= upper)
            break;
    }
    gain = (float) ((float) 64.82 - (float) i / (float) 100);
    return (int) floor(gain * 10.0 + 0.5);
}

/* the title's gain, 0 when no window was completed; the state is ready for the next title afterwards (--nogap) */
int
lh_rg_finish(LhReplayGain * g)
{
    int     tenths;
    if (g->rate_index < 0)
        return 0;
    tenths = lh_rg_tenths(g->bins);
    memset(g->bins, 0, sizeof(g->bins));
    memset(g->hist_in, 0, sizeof(g->hist_in));
    memset(g->hist_mid, 0, sizeof(g->hist_mid));
    memset(g->hist_out, 0, sizeof(g->hist_out));
    g->filled = 0;
    g->lsum = g->rsum = 0.;
    return tenths;
}

/* the gain of a stream from its window sums: `nwin' pairs (lsum, rsum) of windows of `window' samples */
int
lh_gain_from_windows(const double *pairs, long nwin, long window)
{
    uint32_t *bins = (uint32_t *) calloc(LH_RG_BINS, sizeof(uint32_t));
    long    k;
    int     tenths;
    if (!bins)
        return 0;
    for (k = 0; k < nwin; k++)
        bins[lh_rg_bin(pairs[2 * k], pairs[2 * k + 1], window)]++;
    tenths = lh_rg_tenths(bins);
    free(bins);
    return tenths;
}

/* ---- the analysis of a stream fed call by call (an incremental batch), from a cursor of its own ----
 *
 * Without rate conversion lame_encode_buffer hands the analysis a call's samples as they come, in blocks of at most one
 * frame counted from the call's start (reference lame.c:1713-1720): lh_gain_plan_call is one call of m samples at the
 * cursor -- fs, fs, ..., the remainder; none for m == 0 --, lh_gain_plan_flush the bunches of zeros lame_encode_flush feeds
 * until the frames still owed are out (lh_api.cpp).  Both return the number of blocks, write only the first `cap'
 * (blocks == NULL: none) and advance the cursor; -1 for arguments no stream has.  No sample is looked at.  (A batch that
 * converts the rate takes the made counts of lh_rs_plan_call / lh_rs_plan_flush instead: lh_batch.cpp.) */
void
lh_gain_cursor_init(LhGainCursor * c)
{
    c->heard = c->fed = 0;
    c->frames = 0;
}

int
lh_gain_plan_call(LhGainCursor * c, int fs, int mfn, int m, int *blocks, int cap)
{
    int     k = 0, at;
    if (!c || fs < 1 || m < 0)
        return -1;
    for (at = 0; at < m; at += fs) {
        if (blocks && k < cap)
            blocks[k] = m - at > fs ? fs : m - at;
        k++;
    }
    c->heard += m;
    c->fed += m;
    if (LH_MF_START + c->fed >= mfn)
        c->frames = (long) ((LH_MF_START + c->fed - mfn) / fs + 1);
    return k;
}

int
lh_gain_plan_flush(LhGainCursor * c, int fs, int mfn, int *blocks, int cap)
{
    int     k = 0, owed, padding, frames_left;
    if (!c || fs < 1)
        return -1;
    owed = (int) (576 + c->fed - (long long) fs * c->frames);
    padding = fs - (owed % fs);
    if (padding < 576)
        padding += fs;
    frames_left = (owed + padding) / fs;
    while (frames_left > 0) {
        int     bunch = mfn - (int) (LH_MF_START + c->fed - (long long) fs * c->frames);
        bunch = bunch > 1152 ? 1152 : (bunch < 1 ? 1 : bunch);
        if (blocks && k < cap)
            blocks[k] = bunch;
        k++;
        c->fed += bunch;
        c->heard += bunch;
        if (LH_MF_START + c->fed - (long long) fs * c->frames >= mfn) {
            c->frames++;
            frames_left--;
        }
    }
    return k;
}

/* ---- the analysis of a batch's stream as a plan (the device kernel's input, lh_gain.hip) and its host evaluation ----
 *
 * lh_gain_plan: the blocks the handle API hands to lh_rg_block for a stream of n input samples fed `fs' samples per
 * lame_encode_buffer call and flushed, from the length alone.  rs == NULL, no rate conversion: fs samples from position 0
 * on, the remainder, then the flush's bunches of zeros (lh_gain_plan_call per call, lh_gain_plan_flush).  Else the made counts of the
 * stream's conversion plan (lh_rs_plan: trunk, then tail, flush blocks included).  Returns the number of blocks -- only
 * the first `cap' are written --, or -1; *total = the samples they add up to. */
int
lh_gain_plan(const LhResampler * rs, int fs, int mfn, long n, int *blocks, int cap, long *total)
{
    long    sum = 0;
    int     k = 0;
    if (n < 0 || fs < 1)
        return -1;
    if (rs) {
        LhRsBlock one, *b = &one;
        long    conv = 0;
        int     ntrunk = 0, frames = 0, padding = 0, i;
        int const nb = lh_rs_plan(rs, fs, mfn, n, b, 1, &ntrunk, &conv, &frames, &padding);
        if (nb < 0)
            return -1;
        if (nb > 1) {
            b = (LhRsBlock *) malloc((size_t) nb * sizeof(LhRsBlock));
            if (!b || lh_rs_plan(rs, fs, mfn, n, b, nb, &ntrunk, &conv, &frames, &padding) != nb) {
                free(b);
                return -1;
            }
        }
        for (i = 0; i < nb; i++) {
            if (k < cap)
                blocks[k] = b[i].made;
            k++;
            sum += b[i].made;
        }
        if (b != &one)
            free(b);
    }
    else {
        /* a frame's worth per call, then the flush: the call plan's special case */
        LhGainCursor c;
        long    at;
        int     nb;
        lh_gain_cursor_init(&c);
        for (at = 0; at < n; at += fs) {
            nb = lh_gain_plan_call(&c, fs, mfn, (int) (n - at > fs ? fs : n - at), k < cap ? blocks + k : NULL, k < cap ? cap - k : 0);
            if (nb < 0)
                return -1;
            k += nb;
        }
        nb = lh_gain_plan_flush(&c, fs, mfn, k < cap ? blocks + k : NULL, k < cap ? cap - k : 0);
        if (nb < 0)
            return -1;
        k += nb;
        sum = (long) c.heard;
    }
    if (total)
        *total = sum;
    return k;
}

/* lh_gain_eval_host: a plan evaluated on host samples with lh_rg_block's own arithmetic -- the kernel's twin.  l / r: n
 * samples as the analysis hears them (behind the PCM matrix; positions from n on are zeros, generated here); channels == 1:
 * l stands for both.  Writes the first `cap' window pairs, returns the number of windows (or -1) and, with `tenths', the
 * gain. */
long
lh_gain_eval_host(int samplerate, int channels, const int *blocks, int nblocks, const float *l, const float *r, long n,
                  double *pairs, long cap, int *tenths)
{
    LhReplayGain *g = (LhReplayGain *) malloc(sizeof(LhReplayGain));
    float  *buf = (float *) malloc(2 * LH_RG_MAX_BLOCK * sizeof(float));
    long    at = 0, nwin = 0;
    int     i, rc = 0;
    if (!g || !buf || lh_rg_start(g, samplerate) != 0) {
        free(g);
        free(buf);
        return -1;
    }
    for (i = 0; i < nblocks && rc == 0; i++) {
        int const m = blocks[i];
        long    have = n - at;
        if (m <= 0)
            continue;
        if (m > LH_RG_MAX_BLOCK) {
            rc = -1;
            break;
        }
        if (have < 0)
            have = 0;
        if (have > m)
            have = m;
        memset(buf, 0, 2 * LH_RG_MAX_BLOCK * sizeof(float));
        if (have > 0) {
            memcpy(buf, l + at, (size_t) have * sizeof(float));
            if (channels != 1)
                memcpy(buf + LH_RG_MAX_BLOCK, r + at, (size_t) have * sizeof(float));
        }
        rc = rg_block(g, buf, buf + LH_RG_MAX_BLOCK, m, channels, pairs, cap, &nwin);
        at += m;
    }
    if (tenths)
        *tenths = lh_rg_finish(g);
    free(g);
    free(buf);
    return rc ? -1 : nwin;
}
