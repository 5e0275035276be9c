/*
 * lh_pcm_in.c -- the host side of lh_pcm_in.h in plain C: what lh_ingest.hip and the typed rate converter have to
 * reproduce bit for bit.  lamehip_batch_set_input uses lh_pcm_copy_planes; the rest is exported for the tests.
 * Built with -ffp-contract=off like every object of the library.
 */
#include <string.h>
#include "lh_host.h"
#include "lh_pcm_in.h"

/* m[4] = { m00, m01, m10, m11 } of a batch of `type' with the handle's scale / mix / scale_r */
void
lh_pcm_matrix_host(int type, float pcm_scale, float pcm_mix, float pcm_scale_r, float *m)
{
    LhRsMatrix const mx = lh_pcm_matrix(type, pcm_scale, pcm_mix, pcm_scale_r);
    m[0] = mx.m00;
    m[1] = mx.m01;
    m[2] = mx.m10;
    m[3] = mx.m11;
}

static float
pcm_load(int type, const void *p, size_t at)
{
    switch (type) {
    case LH_PCM_S16:
        return (float) ((const int16_t *) p)[at];
    case LH_PCM_S32:
        return (float) ((const int32_t *) p)[at];
    default:
        return ((const float *) p)[at];
    }
}

/* n samples of `type' through the matrix m: l and r advance by `stride' elements per sample; r == NULL: one plane, the
 * second mirrors the first.  Returns 0, or -1 for a type there is none of. */
int
lh_pcm_ingest_host(int type, const float *m, const void *l, const void *r, int stride, long n, float *out_l, float *out_r)
{
    long    i;
    if (type < 0 || type >= LH_PCM_TYPES || stride < 1)
        return -1;
    if (!r)
        r = l;
    for (i = 0; i < n; i++) {
        float const xl = pcm_load(type, l, (size_t) i * (size_t) stride);
        float const xr = pcm_load(type, r, (size_t) i * (size_t) stride);
        out_l[i] = lh_rs_mix(xl, xr, m[0], m[1]);
        out_r[i] = lh_rs_mix(xl, xr, m[2], m[3]);
    }
    return 0;
}

/* n elements of esz bytes from src, every stride-th, into dst (stride 1: a memcpy) */
void
lh_pcm_copy_plane(void *dst, const void *src, int esz, int stride, long n)
{
    long    i;
    if (stride == 1) {
        memcpy(dst, src, (size_t) n * (size_t) esz);
        return;
    }
    if (esz == 2)
        for (i = 0; i < n; i++)
            ((int16_t *) dst)[i] = ((const int16_t *) src)[(size_t) i * (size_t) stride];
    else
        for (i = 0; i < n; i++)
            ((int32_t *) dst)[i] = ((const int32_t *) src)[(size_t) i * (size_t) stride];
}

/* One block of a conversion plan over float planes that are behind the PCM matrix already (lh_pcm_ingest_host),
 * sample by sample as the device kernel does it: zeros before the stream and from n on (lh_rs_eval_block for a
 * typed stream). */
void
lh_pcm_eval_block(const LhResampler * r, const LhRsBlock * b, int channels, const float *xl, const float *xr, long n,
                  float *out_l, float *out_r)
{
    int     k, i;
    for (k = 0; k < b->made; k++) {
        LhRsSpot const s = lh_rs_locate(r->ratio, r->taps, r->phases, b->start, k);
        float   span[2][34];
        for (i = 0; i <= r->taps; i++) {
            long long const at = b->in_at + s.first + i;
            span[0][i] = (at < 0 || at >= n) ? 0.0f : xl[at];
            span[1][i] = (at < 0 || at >= n) ? 0.0f : xr[at];
        }
        out_l[b->out_at + k] = lh_rs_dot(span[0], r->bank[s.kernel], r->taps);
        out_r[b->out_at + k] = channels == 1 ? 0.0f : lh_rs_dot(span[1], r->bank[s.kernel], r->taps);
    }
}
