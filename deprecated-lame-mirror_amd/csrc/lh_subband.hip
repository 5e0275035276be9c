/*
 * lh_subband.hip -- polyphase filterbank + MDCT + alias reduction for all frames of a launch (gfx950).
 *
 * Reference newmdct.c:430-1039 (mdct_sub48) needs, besides the PCM, only the granules' block types, which
 * lh_attack_scan_kernel (lh_analysis.hip) has settled for the whole launch by the time this kernel starts.  A workgroup
 * (wave = channel, as in the fused encode kernel, same arithmetic: lh_dev_mdct.h) takes a run of LH_SB_RUN
 * consecutive frames of one stream: the polyphase output of the granule before the run -- the MDCT overlaps every granule
 * with its predecessor -- is recomputed from the PCM (what the fused kernel does once, on a stream's first frame), inside
 * the run it is kept in LDS.  The spectra go to HBM (LhMidXr), where the encode kernel of the split pipeline
 * (lh_kernels.hip, -DLH_SPLIT) picks them up; the stream's overlap after the launch's last frame goes to
 * LhStreamState.sb_prev, so that the fused kernel could take the stream's next launch.
 *
 * What bounds the kernel is how many waves a SIMD holds, not what they compute (a wave alone issues an instruction every
 * eleven cycles or so: LDS and HBM round trips with nothing to hide behind), so the workgroup is cut to what fits eight
 * times into a CU (lh_lds_subband.h): a wave works on its own channel's plane of LDS alone -- window, sub-band samples and
 * spectra take turns in it, what has to outlive a turn waits in registers -- and meets the other wave at no barrier after
 * the tables are loaded.  The next frame's PCM is on its way from HBM while this frame is transformed.
 */
#include <stdint.h>
#include <math.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_CONST static const
/* (every stage of this kernel is inlined: see lh_dev_math.h) */
#define LH_DEVFN static inline
#define LH_STAGEFN static inline
#define LH_DEVCONST static const
#else
#include <hip/hip_runtime.h>
#define LH_CONST __device__ static const
#define LH_DEVFN __device__ __forceinline__
#define LH_STAGEFN __device__ __forceinline__
#define LH_DEVCONST __device__ static const
#endif

#define LH_CUSTOM_LDS "lh_lds_subband.h"
/* LDS bank conflicts were three quarters of this kernel's LDS time (profiles/r05*): the frame window is stored with bit 4 of
 * the sample index flipped in odd blocks of 32 (lh_dev_mdct.h: LH_MF_SWZ), the time slots of the sub-band samples 33 words apart */
#define LH_MF_SWZ(i) ((i) ^ (((i) >> 1) & 16))
#define LH_SB_STRIDE 33
#define LH_ENW_TAPS (lh_lds.enw)
#define LH_MDCT_WIN (lh_lds.mwin)
#define LH_CUSTOM_MDCT_STAGES   /* lh_sb_polyphase, lh_sb_mdct below */
#include "lh_static_tables.h"
#include "lh_dev_common.h"
#if !defined(LH_EMU)
#define LH_KRESTRICT __restrict__
#else
#define LH_KRESTRICT
#endif

#include "lh_dev_mdct.h"

#if defined(LH_APROF) && !defined(LH_EMU)
#define LH_AP_T0() unsigned long long ap_t = clock64()
#define LH_AP(k) do { unsigned long long const n_ = clock64(); if (c.lane == 0) atomicAdd(&c.st->prof[c.wave][(k)], n_ - ap_t); ap_t = n_; } while (0)
#else
#define LH_AP_T0() do { } while (0)
#define LH_AP(k) do { } while (0)
#endif
#ifndef LH_SB_RUN
#define LH_SB_RUN 16            /* frames per workgroup: one recomputed granule per run */
#endif
#ifndef LH_SB_WAVES
#define LH_SB_WAVES 4           /* waves per SIMD: what the LDS image allows (lh_lds_subband.h) */
#endif
#define LH_SB_PAIRS ((LH_SB_WIN / 2 + 63) / 64)        /* registers that hold a window of 16-bit PCM, two samples each */

#ifdef LH_LSF
#define lh_subband_kernel lh_subband_kernel_lsf
#define lh_launch_subband lh_launch_subband_lsf
#define lh_emu_subband lh_emu_subband_lsf
#endif

/* ---- the window of one channel, staged by its wave alone.  Every sample is what lh_stage_span (lh_dev_common.h) makes of it,
 * from the same three sources. ---- */
struct LhSbSrc {
    float   scale, scale_r, mix;
    long long last;
};

/* sample p of channel ch */
LH_DEVFN float
lh_sb_sample(const LhCtx & c, const LhSbSrc & q, int ch, long long p0)
{
    if (c.pcmf) {
        float   v = 0.0f;
        if (p0 >= 0 && p0 <= q.last && p0 >= c.d.pcm_base)
            v = c.pcmf[(ch == 0 ? c.d.pcm_l : c.d.pcm_r) + (p0 - c.d.pcm_base)];
        return v;
    }
    if (q.mix != 0.0f) {
        float   v = 0.0f;
        if (ch == 0 && p0 >= 0 && p0 <= q.last && p0 >= c.d.pcm_base) {
            float const xl = (float) c.pcm[c.d.pcm_l + (p0 - c.d.pcm_base)];
            float const xr = (float) c.pcm[c.d.pcm_r + (p0 - c.d.pcm_base)];
            v = xl * q.scale + xr * q.mix;
        }
        return v;
    }
    {
        long long p = p0 < 0 ? 0 : (p0 > q.last ? q.last : p0);
        int16_t v;
        p = p < c.d.pcm_base ? c.d.pcm_base : p;        /* never before the pool (also nsamples == 0) */
        v = (c.d.nsamples > 0) ? c.pcm[(ch == 0 ? c.d.pcm_l : c.d.pcm_r) + (p - c.d.pcm_base)] : (int16_t) 0;
        return (p0 < 0 || p0 > q.last) ? 0.0f : (float) v * (ch == 0 ? q.scale : q.scale_r);
    }
}

/* Loads ahead of use: the window that starts at stream sample `base', if it is the usual one -- 16-bit PCM, inside the stream
 * and the pool, on an even element --, is asked for here, two samples per register, and written to LDS by lh_sb_put whenever
 * the plane is free again.  Returns whether it was (wave-uniform). */
LH_DEVFN int
lh_sb_fetch(const LhCtx & c, const LhSbSrc & q, int ch, long long base, uint32_t (&v)[LH_SB_PAIRS])
{
    long long const lo = base, hi = base + LH_SB_WIN - 1;
    long long const o = (ch == 0 ? c.d.pcm_l : c.d.pcm_r) + (base - c.d.pcm_base);
    int const usual = !c.pcmf && q.mix == 0.0f && lo >= 0 && lo >= c.d.pcm_base && hi <= q.last && (o & 1) == 0;
    if (lh_uni_i(usual)) {
        const uint32_t *p = (const uint32_t *) (c.pcm + o);
#pragma unroll
        for (int u = 0; u < LH_SB_PAIRS; u++) {
            int const j = c.lane + 64 * u;
            v[u] = p[j < LH_SB_WIN / 2 ? j : LH_SB_WIN / 2 - 1];
        }
        return 1;
    }
    return 0;
}

LH_DEVFN void
lh_sb_put(const LhCtx & c, const LhSbSrc & q, int ch, long long base, int fetched, const uint32_t (&v)[LH_SB_PAIRS])
{
    float  *mf = lh_lds.mf[ch];
    if (fetched) {
        float const scale = ch == 0 ? q.scale : q.scale_r;
#pragma unroll
        for (int u = 0; u < LH_SB_PAIRS; u++) {
            int const j = c.lane + 64 * u;
            if (j < LH_SB_WIN / 2) {
                lh_f32x2 a;
                a.x = (float) (int16_t) (v[u] & 0xffffu) * scale;
                a.y = (float) (int16_t) (v[u] >> 16) * scale;
                *(lh_f32x2 *) &mf[LH_MF_SWZ(2 * j)] = a;
            }
        }
    }
    else {
        for (int i = c.lane; i < LH_SB_WIN; i += 64)
            mf[LH_MF_SWZ(i)] = lh_sb_sample(c, q, ch, base + i);
    }
}

/* lh_subband_row (lh_dev_mdct.h) for the slot `up' samples (a multiple of 64: it commutes with the swizzle, and all slots of
 * a lane share their four base addresses) after the one at x, with the two tap sums of the row left in registers: the
 * sub-band samples are going to lie where the window lies now */
LH_DEVFN void
lh_sb_row(int ch, int x, int up, int n, const float (&w)[18], float &sum, float &dif)
{
    const float *mf = lh_lds.mf[ch];
    int const x1 = x - n;
    int const x2 = x - 62 + n;
    const float *a2 = mf + LH_MF_SWZ(x2 - 224), *a1 = mf + LH_MF_SWZ(x1 + 224 - 448);
    const float *b1 = mf + LH_MF_SWZ(x1 - 256), *b2 = mf + LH_MF_SWZ(x2 + 256 - 448);
    float   s, t, d;
    s = a2[up] * w[0];
    t = a1[up + 448] * w[0];
#pragma unroll
    for (int k = 1; k < 8; k++) {
        s += a2[up + 64 * k] * w[k];
        t += a1[up + 448 - 64 * k] * w[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        s += b1[up + 64 * k] * w[8 + k];
        t -= b2[up + 448 - 64 * k] * w[8 + k];
    }
    s *= w[16];
    d = t - s;
    sum = t + s;
    dif = w[17] * d;
}

/* lh_subband_centre (lh_dev_mdct.h) with the row's 31 samples read from four base addresses -- one per 16 samples of a block
 * of 64, which is what the swizzle looks at -- at constant offsets, and the results left in registers */
LH_DEVFN void
lh_sb_centre(int ch, int x, float &u, float &v)
{
    const float *mf = lh_lds.mf[ch];
    int const x1 = x - 15;
    const float *wp = LH_ENW_TAPS + 280;
    const float *const q[4] = { mf + LH_MF_SWZ(x1 - 256), mf + LH_MF_SWZ(x1 - 240), mf + LH_MF_SWZ(x1 - 224), mf + LH_MF_SWZ(x1 - 208) };
    float   s, t;
#define LH_MFS(i) q[(((i) + 256) >> 4) & 3][((i) + 256) & ~63]
    t = LH_MFS(-16) * wp[-10];
    s = LH_MFS(-32) * wp[-2];
    t += (LH_MFS(-48) - LH_MFS(16)) * wp[-9];
    s += LH_MFS(-96) * wp[-1];
    t += (LH_MFS(-80) + LH_MFS(48)) * wp[-8];
    s += LH_MFS(-160) * wp[0];
    t += (LH_MFS(-112) - LH_MFS(80)) * wp[-7];
    s += LH_MFS(-224) * wp[1];
    t += (LH_MFS(-144) + LH_MFS(112)) * wp[-6];
    s -= LH_MFS(32) * wp[2];
    t += (LH_MFS(-176) - LH_MFS(144)) * wp[-5];
    s -= LH_MFS(96) * wp[3];
    t += (LH_MFS(-208) + LH_MFS(176)) * wp[-4];
    s -= LH_MFS(160) * wp[4];
    t += (LH_MFS(-240) - LH_MFS(208)) * wp[-3];
    s -= LH_MFS(224);
#undef LH_MFS
    /* u = s - t and v = s + t, combined with rows 14/15 at the start of the butterfly network */
    u = s - t;
    v = s + t;
}

/* lh_polyphase (lh_dev_mdct.h) for this kernel's plane: the 36 slots of the window of channel ch into the plane's two
 * granules of sub-band samples; one wave.  amp_col: the lowpass factor of the band in the lane's storage column. */
LH_DEVFN void
lh_sb_polyphase(const LhCtx & c, int ch, float amp_col)
{
    float   (*sb)[LH_SB_HALF] = lh_lds.u.mdct.sb[ch];
    int const n = c.lane & 15;
    /* stage 1: 36 slots x 16 tap rows.  A lane's units (lane + 64 k) are all at row lane & 15: the fifteen folded rows with their
     * coefficients in registers, the lanes of row 15 sit them out, and the 36 centre rows follow as one trip of 36 lanes */
    float   sum[9], dif[9], cu = 0.0f, cv = 0.0f;
    {
        float   w[18];
#pragma unroll
        for (int k = 0; k < 18; k++)
            w[k] = LH_ENW_TAPS[18 * (n < 15 ? n : 0) + k];
        if (n < 15) {
#pragma unroll
            for (int k = 0; k < 9; k++)
                lh_sb_row(ch, 286 + 32 * (c.lane >> 4), 128 * k, n, w, sum[k], dif[k]);
        }
        if (c.lane < 36)
            lh_sb_centre(ch, 286 + 32 * c.lane, cu, cv);
    }
    LH_WAVE_ORDER();            /* the wave has read its last sample: the plane changes hands */
    if (n < 15) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
            int const s = (c.lane >> 4) + 4 * k;
            int const gr = s / 18, slot = s - gr * 18;
            sb[gr][slot * LH_SB_STRIDE + 2 * n] = sum[k];
            sb[gr][slot * LH_SB_STRIDE + 2 * n + 1] = dif[k];
        }
    }
    if (c.lane < 36) {
        int const s = c.lane;
        int const gr = s / 18, slot = s - gr * 18;
        sb[gr][slot * LH_SB_STRIDE + 30] = cu;
        sb[gr][slot * LH_SB_STRIDE + 31] = cv;
    }
    LH_WAVE_SYNC();
    /* stage 2: butterfly network per slot */
    if (c.lane < 36) {
        int const s = c.lane;
        int const gr = s / 18, slot = s - gr * 18;
        float  *out = &sb[gr][slot * LH_SB_STRIDE];
        lh_subband_network(ch, gr, slot);
        if (slot & 1) {
            /* compensate for the inversion in the analysis filter */
            for (int band = 1; band < 32; band += 2)
                out[band] *= -1;
        }
    }
    LH_WAVE_SYNC();
    /* lowpass: scale each new sub-band sample once.  A lane's storage column is the same on every trip (64 apart); bands the
     * filter leaves alone (factor 1: all below the lowpass) take no trip at all. */
    {
        int const col = c.lane & 31;
        float const a = amp_col;
        if (!(a < 1e-12) && a < 1.0) {
            /* (sample lane + 64 k of either granule: slot (lane >> 5) + 2 k) */
            float  *p = &sb[0][(c.lane >> 5) * LH_SB_STRIDE + col];
#pragma unroll
            for (int k = 0; k < 9; k++) {
                p[2 * k * LH_SB_STRIDE] *= a;
                p[LH_SB_HALF + 2 * k * LH_SB_STRIDE] *= a;
            }
        }
    }
    LH_WAVE_SYNC();
}

/* lh_mdct_granules (lh_dev_mdct.h) for this kernel's plane: MDCT + alias reduction for both granules of channel ch; one wave,
 * lane = granule * 32 + band.  A lane reads its band's 18 samples of its granule and of the one before -- granule 0's
 * predecessor is the one kept from the frame before: LhLds.prev -- before the first spectral line is written over them, and
 * the lanes of the frame's last granule leave in LhLds.prev what the next frame's granule 0 overlaps with.  type0 / type1: the
 * granules' block types; amp_band: the lowpass factor of the lane's band. */
LH_DEVFN void
lh_sb_mdct(const LhCtx & c, int ch, int type0, int type1, float amp_band)
{
    LhLds & L = lh_lds;
    float   (*sb)[LH_SB_HALF] = L.u.mdct.sb[ch];
    int const gr = c.lane >> 5, band = c.lane & 31;
    int const type = gr ? type1 : type0;
    int const col = lh_sb_order[band];
    float  *mdct_enc = &L.xr[ch][gr * 576 + band * 18];
    float   band0[18], band1[18];
    {
        const float *p0 = (gr ? sb[0] : L.prev[ch]) + col, *p1 = sb[gr] + col;
#pragma unroll
        for (int k = 0; k < 18; k++) {
            band0[k] = p0[k * LH_SB_STRIDE];
            band1[k] = p1[k * LH_SB_STRIDE];
        }
    }
    LH_WAVE_ORDER();            /* the sub-band samples are read: the plane changes hands */
    /* (a one-granule frame: the window's second granule is transformed and thrown away) */
    if (gr == LH_NGR - 1) {
#pragma unroll
        for (int k = 0; k < 18; k++)
            L.prev[ch][k * LH_SB_STRIDE + col] = band1[k];
    }
    if (amp_band < 1e-12) {
        for (int k = 0; k < 18; k++)
            mdct_enc[k] = 0.0f;
    }
    else if (type == LH_SHORT_TYPE) {
        float   tmp[18];
#pragma unroll
        for (int k = -3; k < 0; k++) {
            float const w = LH_WIN(LH_SHORT_TYPE, k + 3);
            tmp[k * 3 + 9] = band0[9 + k] * w - band0[8 - k];
            tmp[k * 3 + 18] = band0[14 - k] * w + band0[15 + k];
            tmp[k * 3 + 10] = band0[15 + k] * w - band0[14 - k];
            tmp[k * 3 + 19] = band1[2 - k] * w + band1[3 + k];
            tmp[k * 3 + 11] = band1[3 + k] * w - band1[2 - k];
            tmp[k * 3 + 20] = band1[8 - k] * w + band1[9 + k];
        }
        lh_mdct_short(tmp);
#pragma unroll
        for (int k = 0; k < 18; k++)
            mdct_enc[k] = tmp[k];
    }
    else {
        float   work[18], outv[18];
#pragma unroll
        for (int k = -9; k < 0; k++) {
            float   a, b;
            a = LH_WINV(type, k + 27) * band1[k + 9]
                + LH_WINV(type, k + 36) * band1[8 - k];
            b = LH_WINV(type, k + 9) * band0[k + 9]
                - LH_WINV(type, k + 18) * band0[8 - k];
            work[k + 9] = a - b * LH_TANTAB(k + 9);
            work[k + 18] = a * LH_TANTAB(k + 9) + b;
        }
        lh_mdct_long(outv, work);
#pragma unroll
        for (int k = 0; k < 18; k++)
            mdct_enc[k] = outv[k];
    }
    LH_WAVE_SYNC();
    /* aliasing reduction butterflies: pairs (band*18 + k, band*18 - 1 - k), band 1..31, k 0..7 */
    for (int t = c.lane; t < 2 * 31 * 8; t += 64) {
        int const g = t / (31 * 8), r = t - g * (31 * 8);
        int const bnd = 1 + r / 8, k = r & 7;
        if ((g ? type1 : type0) != LH_SHORT_TYPE) {
            float  *p = &L.xr[ch][g * 576 + bnd * 18];
            float   bu, bd;
            float const ca = LH_WINV(LH_SHORT_TYPE, 20 + k), cs = LH_WINV(LH_SHORT_TYPE, 28 + k);
            bu = p[k] * ca + p[-1 - k] * cs;
            bd = p[k] * cs - p[-1 - k] * ca;
            p[-1 - k] = bu;
            p[k] = bd;
        }
    }
    LH_WAVE_SYNC();
}

#ifndef LH_EMU
extern "C" __global__ void __launch_bounds__(LH_NT, LH_SB_WAVES)
#else
void
#endif
lh_subband_kernel(const LhConfig * LH_KRESTRICT cfg, const LhTables * LH_KRESTRICT T, const int16_t * LH_KRESTRICT pcm, const float *pcmf, const LhStreamDesc * descs,
                  LhStreamState * states, LhMidFrame * frames, int nstreams)
{
    LhLds & L = lh_lds;
    int const sidx = (int) blockIdx.y;
    constexpr int ngr = LH_NGR, fs = 576 * LH_NGR;
    LhCtx   c;
    c.cfg = cfg;
    c.T = T;
    c.st = &states[sidx];
    c.pcm = pcm;
    c.pcmf = pcmf;
    c.d = descs[sidx];
    c.d.pcm_l = lh_uni_ll(c.d.pcm_l);
    c.d.pcm_r = lh_uni_ll(c.d.pcm_r);
    c.d.pcm_base = lh_uni_ll(c.d.pcm_base);
    c.d.nsamples = lh_uni_ll(c.d.nsamples);
    c.d.out_index = lh_uni_ll(c.d.out_index);
    c.d.mid_rel = lh_uni_i(c.d.mid_rel);
    c.d.frame_begin = lh_uni_i(c.d.frame_begin);
    c.d.frame_end = lh_uni_i(c.d.frame_end);
    c.tid = (int) threadIdx.x;
    c.lane = c.tid & 63;
    c.wave = lh_uni_i(c.tid >> 6);
    int const f0 = c.d.frame_begin + LH_SB_RUN * (int) blockIdx.x;
    int const f1 = (f0 + LH_SB_RUN < c.d.frame_end) ? f0 + LH_SB_RUN : c.d.frame_end;
    if (f0 >= c.d.frame_end)
        return;
    int const w = c.wave, lane = c.lane, tid = c.tid;
    LhSbSrc q;
    q.scale = c.cfg->pcm_scale;
    q.scale_r = c.cfg->pcm_scale_r;
    q.mix = c.cfg->pcm_mix;
    q.last = c.d.nsamples - 1;
    /* the lowpass factors this lane needs: of the band in its storage column (the column order -- bits 1..4 of the band
     * reversed -- is its own inverse) and of its band */
    float const amp_col = c.T->amp_filter[lh_sb_order[lane & 31]], amp_band = c.T->amp_filter[lane & 31];
    uint32_t pv[LH_SB_PAIRS];
    int     fetched;
    LH_AP_T0();
    /* the granule before the run (reference encoder.c:189-236 primes the filterbank the same way on a stream's first frame) */
    long long base = (long long) fs * f0 - LH_MF_START - fs;
    fetched = lh_sb_fetch(c, q, w, base, pv);
    for (int i = tid; i < 288; i += LH_NT)
        L.enw[i] = lh_enwindow[i < 285 ? i : 284];
    for (int i = tid; i < 4 * 36; i += LH_NT)
        L.mwin[i] = lh_mdct_win[i];
    lh_sb_put(c, q, w, base, fetched, pv);
    base += fs;
    fetched = lh_sb_fetch(c, q, w, base, pv);
    LH_SYNC_WG_LDS();           /* the tables; from here on a wave works on its own plane alone */
    lh_sb_polyphase(c, w, amp_col);
    for (int i = lane; i < LH_SB_GRANULE; i += 64)
        L.prev[w][i] = L.u.mdct.sb[w][ngr - 1][i];
    LH_WAVE_ORDER();
    LH_AP(8);
    for (int f = f0; f < f1; f++) {
        long long const at = c.d.out_index + c.d.mid_rel + (f - c.d.frame_begin);
        /* (a one-granule frame: the transforms also run over the window's second granule, which is thrown away) */
        int const type0 = lh_uni_i((int) frames[at].small.gr[0].block_type[w]);
        int const type1 = ngr > 1 ? lh_uni_i((int) frames[at].small.gr[ngr - 1].block_type[w]) : LH_NORM_TYPE;
        lh_sb_put(c, q, w, base, fetched, pv);
        base += fs;
        fetched = (f + 1 < f1) ? lh_sb_fetch(c, q, w, base, pv) : 0;
        LH_WAVE_SYNC();
        LH_AP(9);
        lh_sb_polyphase(c, w, amp_col);
        LH_AP(10);
        lh_sb_mdct(c, w, type0, type1, amp_band);
        LH_AP(11);
        {
            lh_f32x4 *dst = (lh_f32x4 *) frames[at].xr.xr + 288 * w;
            const lh_f32x4 *src = (const lh_f32x4 *) L.xr[w];
            for (int i = lane; i < 288; i += 64)
                dst[i] = src[i];
        }
        LH_WAVE_ORDER();        /* the spectra are read before the next window is written over them */
        LH_AP(12);
    }
    if (f1 == c.d.frame_end) {
        /* the stream's overlap after the launch (LhStreamState keeps the plain layout: slot * 32 + band) */
        for (int i = lane; i < 18 * 32; i += 64)
            c.st->sb_prev[w][i] = L.prev[w][(i >> 5) * LH_SB_STRIDE + (i & 31)];
    }
}

#ifndef LH_EMU
extern "C" int
lh_launch_subband(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf, const LhStreamDesc * descs,
                  LhStreamState * states, LhMidPools mid, int nstreams, int max_frames, void *stream)
{
    if (nstreams <= 0 || max_frames <= 0)
        return 0;
    hipLaunchKernelGGL(lh_subband_kernel, dim3((unsigned) ((max_frames + LH_SB_RUN - 1) / LH_SB_RUN), (unsigned) nstreams),
                       dim3(LH_NT), 0, (hipStream_t) stream, cfg, T, pcm, pcmf, descs, states, mid.frames, nstreams);
    return (int) hipGetLastError();
}
#else
extern "C" int
lh_emu_subband(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf, const LhStreamDesc * descs,
               LhStreamState * states, const LhMidPools * pools, int nstreams, int max_frames)
{
    LhMidPools const mid = *pools;
    hipemu_dim3 grid = { (unsigned) ((max_frames + LH_SB_RUN - 1) / LH_SB_RUN), (unsigned) nstreams, 1 }, block = { LH_NT, 1, 1 };
    hipemu_run(grid, block,[=] () {
               lh_subband_kernel(cfg, T, pcm, pcmf, descs, states, mid.frames, nstreams);
               }
    );
    return 0;
}
#endif
