/*
 * lh_resample.c -- input rate -> output rate conversion in front of the batched encoder (host C).
 *
 * What has to come out: exactly the float samples the reference's converter produces (reference
 * util.c:483-697 -- a polyphase bank of Blackman-windowed sinc kernels, the kernel of an output
 * sample picked by the fractional part of its input time), because the bytes downstream are
 * compared with the reference's.  The arithmetic (which products are float, which double, and the
 * order of every sum) is therefore fixed by the reference; the organisation here is this file's own:
 *
 *   - a converter is a `kernel bank' (designed once: lh_rs_init) plus, per channel, a `tail' of the
 *     last input samples and the input time at which the next block starts;
 *   - a block (lh_rs_block) sees the channel's signal as ONE virtual sequence, tail followed by the
 *     new input (rs_at), locates each output sample on it (rs_locate), gathers the span of input
 *     the kernel covers and takes the ordered dot product (rs_dot);
 *   - afterwards the tail is simply the last keep samples of that same virtual sequence.
 *
 * A batch converts whole streams: lh_rs_convert_stream strings the blocks together the way the reference's
 * frontend would have them, and lh_rs_plan* says which blocks those are without looking at a sample -- what
 * the device conversion (lh_resample_dev.hip) works from; the per-sample arithmetic both share is
 * lh_rs_sample.h.
 *
 * The reference re-bases its input time once per fill_buffer block, and which kernel a sample gets
 * depends on that rounding, so blocks must be cut where the reference cuts them: the handle API
 * strings them together the way lame_encode_buffer / lame_encode_flush do (lh_api.cpp).
 * Built with -ffp-contract=off.
 */
#include <math.h>
#include <float.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"

static const double rs_pi = 3.14159265358979323846;

/* inputs within +-0.05 % of the output rate pass through unconverted (reference util.c:658) */
int
lh_rs_needed(int rate_in, int rate_out)
{
    int const band_lo = rate_out * 0.9995f, band_hi = rate_out * 1.0005f;
    return !(band_lo <= rate_in && rate_in <= band_hi);
}

/* kernels per unit of input time = rate_out / gcd(rate_out, rate_in), at most LH_RS_MAXPHASES */
static int
rs_phase_count(int rate_in, int rate_out)
{
    int     a = rate_out, b = rate_in, n;
    while (b != 0) {
        int const rest = a % b;
        a = b;
        b = rest;
    }
    n = rate_out / a;
    return n < LH_RS_MAXPHASES ? n : LH_RS_MAXPHASES;
}

/* Design kernel `ph' of the bank: tap i sits at i - shift on a window of `span' input samples,
 * shift = (ph - phases) / (2 phases) in [-1/2, +1/2].  Window and sinc are evaluated in the
 * reference's precision mix (position and cut-off are floats, the trigonometry is double), and
 * the taps are normalised by their float sum in tap order. */
static void
rs_design_kernel(LhResampler * r, int ph, float cutoff)
{
    int const span = r->taps;
    float const shift = (float) ((ph - r->phases) / (2. * r->phases));
    float const wc = (float) (rs_pi * cutoff);
    float  *tap = r->bank[ph];
    float   total = 0.f;
    int     i;
    for (i = 0; i <= span; i++) {
        float   u = i - shift, centre, value;
        u /= span;
        u = (u < 0) ? 0 : (u > 1) ? 1 : u;     /* position on the window, 0..1 */
        centre = (float) (u - .5);
        if (fabs(centre) < 1e-9)
            value = (float) (wc / rs_pi);
        else {
            float const blackman = (float) (0.42 - 0.5 * cos(2 * u * rs_pi) + 0.08 * cos(4 * u * rs_pi));
            value = (float) (blackman * sin(span * wc * centre) / (rs_pi * span * centre));
        }
        tap[i] = value;
        total += value;
    }
    for (i = 0; i <= span; i++)
        tap[i] /= total;
}

void
lh_rs_init(LhResampler * r, int rate_in, int rate_out)
{
    float   cutoff;
    int     whole, ph;
    memset(r, 0, sizeof(*r));
    r->rate_in = rate_in;
    r->rate_out = rate_out;
    r->ratio = (double) rate_in / (double) rate_out;
    r->phases = rs_phase_count(rate_in, rate_out);
    /* an odd span of 31, or 32 when every output sample falls on an input sample */
    whole = fabs(r->ratio - floor(.5 + r->ratio)) < FLT_EPSILON;
    r->taps = whole ? 32 : 31;
    cutoff = (float) (1.00 / r->ratio);
    if (cutoff > 1.00)
        cutoff = 1.00;
    for (ph = 0; ph <= 2 * r->phases; ph++)
        rs_design_kernel(r, ph, cutoff);
}

/* The converter of a stream the reference does not convert (lh_rs_needed == 0: the input rate is the output rate, or
 * within 0.05 % of it), for the plans below only: no bank, taps == 0 marks it, and the ratio is the 1 that
 * lame_encode_flush uses when it does not resample.  Its blocks are what fill_buffer takes (reference util.c:913-920):
 * min(frame size, samples at hand), made = used. */
void
lh_rs_init_identity(LhResampler * r, int rate_in, int rate_out)
{
    memset(r, 0, sizeof(*r));
    r->rate_in = rate_in;
    r->rate_out = rate_out;
    r->ratio = 1.0;
}

int
lh_rs_is_identity(const LhResampler * r)
{
    return r->taps == 0;
}

/* sample `at' of the channel's virtual sequence: negative positions are the tail kept from the
 * previous blocks (its last sample is position -1) */
static float
rs_at(const float *tail, int keep, const float *in, int at)
{
    return at < 0 ? tail[keep + at] : in[at];
}

/* where output sample k of the block sits, and the ordered dot product: lh_rs_sample.h (shared with the device) */
static LhRsSpot
rs_locate(const LhResampler * r, double start, int k)
{
    return lh_rs_locate(r->ratio, r->taps, r->phases, start, k);
}

/* dot product of the span starting at `first' with one kernel, in tap order */
static float
rs_dot(const LhResampler * r, const float *tail, const float *in, LhRsSpot s)
{
    float   span[34];
    int     i;
    for (i = 0; i <= r->taps; ++i)
        span[i] = rs_at(tail, r->taps + 1, in, s.first + i);
    return lh_rs_dot(span, r->bank[s.kernel], r->taps);
}

/* One block: up to `want' output samples of channel ch from in[0..len), continuing after the
 * previous blocks.  Returns the number written; *used = input samples consumed. */
int
lh_rs_block(LhResampler * r, int ch, float *out, int want, const float *in, int len, int *used)
{
    int const keep = r->taps + 1;
    float  *tail = r->history[ch];
    double const start = r->clock[ch];
    int     made = 0, reach = r->taps - r->taps / 2, taken, i;

    while (made < want) {
        LhRsSpot const s = rs_locate(r, start, made);
        reach = s.first + r->taps;      /* last input position the span touches */
        if (reach >= len)
            break;              /* the kernel reaches past the input at hand */
        out[made++] = rs_dot(r, tail, in, s);
    }
    /* The reference measures consumption by the span of the sample it stopped at (made or not);
     * with no sample attempted (want == 0) that is the span of position 0. */
    taken = (len < reach) ? len : reach;
    *used = taken;
    /* next block: its output 0 is due at time 0, its input begins at clock[ch] */
    r->clock[ch] = start + (taken - made * r->ratio);
    /* new tail = the last `keep' samples of [tail | in[0..taken)] */
    {
        float   next[34];
        for (i = 0; i < keep; i++)
            next[i] = rs_at(tail, keep, in, taken - keep + i);
        memcpy(tail, next, (size_t) keep * sizeof(float));
    }
    return made;
}

/* ---- a whole stream, the way a batch converts it ---------------------------------------------
 * What the reference makes of a stream when its frontend feeds lame_encode_buffer fs input samples at a time
 * and then flushes (lame.c:1708-1772, 2075-2120): every call is cut into blocks of at most one frame of
 * output, a frame is counted whenever the buffered samples reach mfn, and the flush feeds zeros in bunches
 * sized to complete one frame each until the frames owed (converter delay included) are out. */

void
lh_rs_free(void *p)
{
    free(p);
}

/* frames still owed and the end padding once the input is through (fed = output samples so far); ratio 0: a stream that
 * is not converted, which owes nothing for the converter's delay (reference lame.c:2075-2083) */
static int
rs_frames_left(double ratio, int fs, long long fed, int frames, int *padding)
{
    int     owed = (int) (576 + fed - (long long) fs * frames);
    if (ratio > 0)
        owed += 16. / ratio;
    *padding = fs - (owed % fs);
    if (*padding < 576)
        *padding += fs;
    return (owed + *padding) / fs;
}

/* input samples of the next flush bunch */
static int
rs_flush_bunch(double ratio, int mfn, long mf_size)
{
    int     bunch = (int) (mfn - mf_size);
    bunch *= ratio;
    if (bunch > 1152)
        bunch = 1152;
    if (bunch < 1)
        bunch = 1;
    return bunch;
}

typedef struct {
    float  *v[2];
    long    n, cap;
} RsOut;

static int
rs_out_room(RsOut * o, long more)
{
    int     ch;
    if (o->n + more <= o->cap)
        return 0;
    o->cap = (o->n + more) * 2 + 4096;
    for (ch = 0; ch < 2; ch++) {
        float  *bigger = (float *) realloc(o->v[ch], (size_t) o->cap * sizeof(float));
        if (!bigger)
            return -1;
        o->v[ch] = bigger;
    }
    return 0;
}

int
lh_rs_convert_stream(LhResampler * r, int rate_in, int rate_out, int fs, int mfn, int channels, float pcm_scale, float pcm_mix,
                     float pcm_scale_r, const short *l, const short *rr, long n, float **out_l, float **out_r, long *conv_len,
                     int *frames_out, int *padding_out)
{
    RsOut   o = { {0, 0}, 0, 0 };
    float   in[2][1152], blk[2][1152];
    LhRsMatrix const mx = lh_rs_matrix(pcm_scale, pcm_mix, pcm_scale_r);
    long long fed = 0;
    long    mf_size = LH_MF_START, pos;
    int     frames = 0, padding = 0, frames_left, flushing = 0, m, i, ch;

    *out_l = *out_r = 0;
    if (fs > 1152 || n < 0)
        return -1;
    if (channels == 1 && pcm_mix == 0.0f)
        rr = l;                 /* mono without a downmix: the second plane is not looked at */
    lh_rs_init(r, rate_in, rate_out);
    if (rs_out_room(&o, (long) ((double) n / r->ratio) + 4096) != 0)
        goto fail;
    pos = 0;
    frames_left = 0;
    for (;;) {
        int     at = 0;
        if (!flushing && pos < n) {
            m = (n - pos) > fs ? fs : (int) (n - pos);
            for (i = 0; i < m; i++) {
                float const xl = (float) l[pos + i], xr = (float) rr[pos + i];
                in[0][i] = lh_rs_mix(xl, xr, mx.m00, mx.m01);
                in[1][i] = lh_rs_mix(xl, xr, mx.m10, mx.m11);
            }
            pos += m;
        }
        else {
            if (!flushing) {
                flushing = 1;
                frames_left = rs_frames_left(r->ratio, fs, fed, frames, &padding);
                memset(in, 0, sizeof(in));
            }
            if (frames_left <= 0)
                break;
            m = rs_flush_bunch(r->ratio, mfn, mf_size);
        }
        {
            int const before = frames;
            while (m > 0) {
                int     used = 0, made = 0;
                for (ch = 0; ch < channels; ch++)
                    made = lh_rs_block(r, ch, blk[ch], fs, in[ch] + at, m, &used);
                if (channels == 1)
                    memset(blk[1], 0, sizeof(blk[1]));
                if (rs_out_room(&o, made) != 0)
                    goto fail;
                memcpy(o.v[0] + o.n, blk[0], (size_t) made * sizeof(float));
                memcpy(o.v[1] + o.n, blk[1], (size_t) made * sizeof(float));
                o.n += made;
                fed += made;
                mf_size += made;
                if (mf_size >= mfn) {
                    frames++;
                    mf_size -= fs;
                }
                at += used;
                m -= used;
            }
            if (flushing)
                frames_left -= (frames != before) ? 1 : 0;
        }
    }
    *out_l = o.v[0];
    *out_r = o.v[1];
    *conv_len = o.n;
    *frames_out = frames;
    *padding_out = padding;
    return 0;
  fail:
    free(o.v[0]);
    free(o.v[1]);
    return -1;
}

/* ---- the same conversion as a plan ----------------------------------------------------------
 * Which blocks there are, and each block's len / made / used / clock, follows from the rates, the frame size
 * and the stream's length alone: lh_rs_block stops at the first output sample whose span reaches the end of
 * the input at hand, and floor(k ratio - start) is monotone in k, so that sample is found from an estimate
 * corrected at its neighbours with the exact expression (rs_locate) instead of by walking the samples. */

/* last input position the span of output sample k touches */
static int
rs_reach(const LhResampler * r, double start, int k)
{
    return rs_locate(r, start, k).first + r->taps;
}

/* what lh_rs_block(want, len) makes and consumes at clock `start' */
static void
rs_block_extent(const LhResampler * r, double start, int want, int len, int *made, int *taken)
{
    int     reach = r->taps - r->taps / 2, k;
    if (lh_rs_is_identity(r)) {
        /* not converted: fill_buffer's copy */
        *made = *taken = len < want ? len : want;
        return;
    }
    if (want > 0) {
        /* smallest k with rs_reach(k) >= len, i.e. floor(k ratio - start) >= len - taps + taps / 2 */
        double const guess = ceil((len - r->taps + r->taps / 2 + start) / r->ratio);
        k = guess < 0 ? 0 : guess > want ? want : (int) guess;
        while (k > 0 && rs_reach(r, start, k - 1) >= len)
            k--;
        while (k < want && rs_reach(r, start, k) < len)
            k++;
        /* k == want: every sample was made, the loop stopped behind the last one's span */
        reach = rs_reach(r, start, k < want ? k : want - 1);
    }
    else
        k = 0;
    *made = k;
    *taken = (len < reach) ? len : reach;
}

typedef struct {
    LhRsBlock *blk;
    long    cap, n;
} RsList;

/* one lame_encode_buffer call of m input samples at the cursor: its blocks go to `list' (counted beyond its
 * capacity, not written) */
static void
rs_plan_feed(const LhResampler * r, int fs, int mfn, LhRsCursor * c, int m, RsList * list)
{
    while (m > 0) {
        int     made, used;
        rs_block_extent(r, c->clock, fs, m, &made, &used);
        if (list->n < list->cap) {
            LhRsBlock *b = &list->blk[list->n];
            b->in_at = c->in_at;
            b->out_at = c->fed;
            b->start = c->clock;
            b->len = m;
            b->made = made;
        }
        list->n++;
        c->nblk++;
        c->clock = c->clock + (used - made * r->ratio);
        c->in_at += used;
        c->fed += made;
        c->mf_size += made;
        if (c->mf_size >= mfn) {
            c->frames++;
            c->mf_size -= fs;
        }
        m -= used;
    }
}

void
lh_rs_trunk_init(LhRsTrunk * t, int fs, int mfn)
{
    memset(t, 0, sizeof(*t));
    t->fs = fs;
    t->mfn = mfn;
}

void
lh_rs_trunk_free(LhRsTrunk * t)
{
    free(t->after);
    free(t->blk);
    t->after = 0;
    t->blk = 0;
    t->nchunks = t->cap_chunks = t->cap_blk = 0;
}

int
lh_rs_trunk_extend(const LhResampler * r, LhRsTrunk * t, long nchunks)
{
    if (nchunks + 1 > t->cap_chunks) {
        long const cap = 2 * nchunks + 64;
        LhRsCursor *bigger = (LhRsCursor *) realloc(t->after, (size_t) cap * sizeof(LhRsCursor));
        if (!bigger)
            return -1;
        t->after = bigger;
        t->cap_chunks = cap;
    }
    if (t->nchunks == 0) {
        memset(&t->after[0], 0, sizeof(t->after[0]));
        t->after[0].mf_size = LH_MF_START;
    }
    while (t->nchunks < nchunks) {
        LhRsCursor c = t->after[t->nchunks];
        RsList  list;
        /* a block makes a frame of output (from fs * ratio input samples) or takes all the input left: room for the
         * chunk's worst case before it is planned */
        long const worst = (long) (1.0 / r->ratio) + 8;
        if (c.nblk + worst > t->cap_blk) {
            long const cap = 2 * (c.nblk + worst) + 256;
            LhRsBlock *bigger = (LhRsBlock *) realloc(t->blk, (size_t) cap * sizeof(LhRsBlock));
            if (!bigger)
                return -1;
            t->blk = bigger;
            t->cap_blk = cap;
        }
        list.blk = t->blk + c.nblk;
        list.cap = t->cap_blk - c.nblk;
        list.n = 0;
        rs_plan_feed(r, t->fs, t->mfn, &c, t->fs, &list);
        if (list.n > list.cap)
            return -1;
        t->after[++t->nchunks] = c;
    }
    return 0;
}

int
lh_rs_plan_tail(const LhResampler * r, const LhRsTrunk * t, long n, LhRsBlock * tail, int cap, long *conv_len, int *frames,
                int *padding)
{
    long const chunks = n / t->fs;
    LhRsCursor c;
    RsList  list;
    int     frames_left;
    if (n < 0 || chunks > t->nchunks)
        return -1;
    c = t->after[chunks];
    list.blk = tail;
    list.cap = cap;
    list.n = 0;
    if (n > chunks * t->fs)
        rs_plan_feed(r, t->fs, t->mfn, &c, (int) (n - chunks * t->fs), &list);
    frames_left = rs_frames_left(r->ratio, t->fs, c.fed, c.frames, padding);
    while (frames_left > 0) {
        int const before = c.frames;
        rs_plan_feed(r, t->fs, t->mfn, &c, rs_flush_bunch(r->ratio, t->mfn, c.mf_size), &list);
        frames_left -= (c.frames != before) ? 1 : 0;
    }
    *conv_len = (long) c.fed;
    *frames = c.frames;
    return (int) list.n;
}

int
lh_rs_plan(const LhResampler * r, int fs, int mfn, long n, LhRsBlock * out, int cap, int *ntrunk, long *conv_len, int *frames,
           int *padding)
{
    LhRsTrunk t;
    int     ntail, k;
    lh_rs_trunk_init(&t, fs, mfn);
    if (n < 0 || lh_rs_trunk_extend(r, &t, n / fs) != 0) {
        lh_rs_trunk_free(&t);
        return -1;
    }
    k = t.after[n / fs].nblk;
    *ntrunk = k;
    if (k > 0 && k <= cap)
        memcpy(out, t.blk, (size_t) k * sizeof(LhRsBlock));
    ntail = lh_rs_plan_tail(r, &t, n, k <= cap ? out + k : out, k <= cap ? cap - k : 0, conv_len, frames, padding);
    lh_rs_trunk_free(&t);
    return ntail < 0 ? -1 : k + ntail;
}

/* ---- the plan of a stream that is fed call by call (an incremental batch) -------------------------
 * Where the reference cuts its blocks depends on how lame_encode_buffer was called, so this plan follows the calls:
 * a cursor per stream, advanced by every call and at last by the flush.  The arithmetic is rs_plan_feed's, the same the
 * whole-stream plan above is made of. */

void
lh_rs_cursor_init(LhRsCursor * c)
{
    memset(c, 0, sizeof(*c));
    c->mf_size = LH_MF_START;
}

int
lh_rs_plan_call(const LhResampler * r, int fs, int mfn, LhRsCursor * c, int m, LhRsBlock * blk, int cap)
{
    RsList  list;
    list.blk = blk;
    list.cap = blk ? cap : 0;
    list.n = 0;
    rs_plan_feed(r, fs, mfn, c, m, &list);
    return (int) list.n;
}

int
lh_rs_plan_flush(const LhResampler * r, int fs, int mfn, LhRsCursor * c, LhRsBlock * blk, int cap, int *padding)
{
    RsList  list;
    int     frames_left = rs_frames_left(lh_rs_is_identity(r) ? 0 : r->ratio, fs, c->fed, c->frames, padding);
    list.blk = blk;
    list.cap = blk ? cap : 0;
    list.n = 0;
    while (frames_left > 0) {
        int const before = c->frames;
        rs_plan_feed(r, fs, mfn, c, rs_flush_bunch(r->ratio, mfn, c->mf_size), &list);
        frames_left -= (c->frames != before) ? 1 : 0;
    }
    return (int) list.n;
}

/* input positions outputs [k0, k0 + count) of a block touch, first tap of the first to last tap of the last */
static int
rs_tile_span(const LhResampler * r, double start, int k0, int count)
{
    return rs_reach(r, start, k0 + count - 1) + 1 - rs_locate(r, start, k0).first;
}

int
lh_rs_block_tiles(const LhResampler * r, const LhRsBlock * b, int stream, LhRsTile * tiles, int cap)
{
    return lh_rs_block_tiles_class(r, b, stream, 0, tiles, cap);
}

int
lh_rs_block_tiles_class(const LhResampler * r, const LhRsBlock * b, int stream, int cls, LhRsTile * tiles, int cap)
{
    /* (floor(k ratio - start) is monotone in k, so a tile's span is in its count: an estimate from the ratio, corrected
     * with the exact expression) */
    double const guess = (LH_RS_SPAN_MAX - r->taps - 1) / r->ratio;
    int const whole = lh_rs_is_identity(r);     /* (a copy stages nothing: the block is one tile) */
    int     k0 = 0, n = 0;
    while (k0 < b->made) {
        int const left = b->made - k0;
        int     count = whole ? left : guess < 1 ? 1 : guess > left ? left : (int) guess;
        while (!whole && count > 1 && rs_tile_span(r, b->start, k0, count) > LH_RS_SPAN_MAX)
            count--;
        while (!whole && count < left && rs_tile_span(r, b->start, k0, count + 1) <= LH_RS_SPAN_MAX)
            count++;
        if (tiles && n < cap) {
            LhRsTile *t = &tiles[n];
            t->in_at = b->in_at;
            t->out_at = b->out_at + k0;
            t->start = b->start;
            t->k0 = k0;
            t->count = count;
            t->stream = stream;
            t->cls = cls;
        }
        n++;
        k0 += count;
    }
    return n;
}

/* input sample `at' (absolute) of the stream behind the PCM matrix: zero outside [0, n) */
static void
rs_input(const LhRsMatrix * mx, const short *l, const short *rr, long n, long long at, float *xl_out, float *xr_out)
{
    if (at < 0 || at >= n)
        *xl_out = *xr_out = 0.0f;
    else {
        float const xl = (float) l[at], xr = (float) rr[at];
        *xl_out = lh_rs_mix(xl, xr, mx->m00, mx->m01);
        *xr_out = lh_rs_mix(xl, xr, mx->m10, mx->m11);
    }
}

void
lh_rs_eval_block(const LhResampler * r, const LhRsBlock * b, int channels, float pcm_scale, float pcm_mix, float pcm_scale_r,
                 const short *l, const short *rr, long n, float *out_l, float *out_r)
{
    LhRsMatrix const mx = lh_rs_matrix(pcm_scale, pcm_mix, pcm_scale_r);
    int     k, i;
    if (channels == 1 && pcm_mix == 0.0f)
        rr = l;
    for (k = 0; k < b->made; k++) {
        LhRsSpot const s = rs_locate(r, b->start, k);
        float   span[2][34];
        for (i = 0; i <= r->taps; i++)
            rs_input(&mx, l, rr, n, b->in_at + s.first + i, &span[0][i], &span[1][i]);
        out_l[b->out_at + k] = lh_rs_dot(span[0], r->bank[s.kernel], r->taps);
        out_r[b->out_at + k] = channels == 1 ? 0.0f : lh_rs_dot(span[1], r->bank[s.kernel], r->taps);
    }
}
