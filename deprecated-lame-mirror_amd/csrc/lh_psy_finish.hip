/*
 * lh_psy_finish.hip -- the masking under its recurrences, taken off the encode kernel's serial chain (gfx950).
 *
 * What the analysis kernels (lh_analysis.hip) leave of a granule's masking are the partition energies before the
 * recurrences (LhMidMask); the encode kernel of the split pipeline used to finish them frame after frame: the pre-echo
 * clamp against the two previous long calls, the masking adjustment, the mid/side thresholds under the ATH level, the sums
 * over the scalefactor bands (stages 6 - 8 of lh_psy_granule).  In a CBR or ABR launch none of that depends on the
 * quantiser: the masking adjustment a frame's model sees follows from the previous frame's block types, the clamp's two
 * previous calls are the neighbouring granules' records, and the ATH level follows the loudness alone.  So for such
 * launches (MPEG-1 streams) the kernels of this file do it for all granules of the launch at once and leave the band
 * energies / thresholds in HBM (lh_device.h: LhMidPsy), where the encode kernel's frame prologue picks them up.
 *
 *   lh_ath_scan_kernel   (stream): the ATH level, the masking adjustment and the block-type state each frame's model sees --
 *                        the recurrences proper, two loudness values and four flags per frame
 *   lh_psy_mask_kernel   (stream, granule): stages 6 - 8, the same device functions as the encode kernel's
 *                        (lh_dev_psy_core.h: lh_psy_stage_mask / _bands / _short), bit-identical results
 *
 * The VBR loops feed the frame's perceptual entropy back into the masking adjustment: they keep the encode kernel's path.
 */
#include <stdint.h>
#include <math.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_CONST static const
#else
#include <hip/hip_runtime.h>
#define LH_CONST __device__ static const
#endif

#define LH_PSY_FINISH
#define LH_CUSTOM_LDS "lh_lds_psyfin.h"
#define LH_CUSTOM_SMP
#include "lh_static_tables.h"
#include "lh_dev_common.h"
#if !defined(LH_EMU)
#define LH_KRESTRICT __restrict__
#else
#define LH_KRESTRICT
#endif

/* (the transforms of lh_dev_psy_core.h read the PCM window through this; none of them is called here) */
LH_DEVFN float
lh_smp(const LhCtx &, int, int)
{
    return 0.0f;
}

#include "lh_dev_psy_core.h"

/* where stages 6 - 8 find things in this file's LDS image */
struct LhPsyAt {
    LH_DEVMEM float *eb(int chn) const { return &lh_lds.eb[chn * 64]; }
    LH_DEVMEM float *thr(int chn) const { return &lh_lds.thr[chn * 64]; }
    LH_DEVMEM float *en(int chn) const { return &lh_lds.en[chn][0]; }
    LH_DEVMEM float *thm(int chn) const { return &lh_lds.thm[chn][0]; }
    LH_DEVMEM int uselong(int ch) const { return lh_lds.uselong[ch]; }
};

LH_DEVFN LhStreamDesc
lh_desc_uniform(const LhStreamDesc * descs, int sidx)
{
    LhStreamDesc d = descs[sidx];
    d.out_index = lh_uni_ll(d.out_index);
    d.mid_rel = lh_uni_i(d.mid_rel);
    d.frame_begin = lh_uni_i(d.frame_begin);
    d.frame_end = lh_uni_i(d.frame_end);
    return d;
}

/* blocktype_old after a granule whose channel keeps long blocks (ul) or not (reference psymodel.c:1289-1319) */
LH_DEVFN int
lh_blocktype_next(int was, int ul)
{
    return ul ? (was == LH_SHORT_TYPE ? LH_STOP_TYPE : LH_NORM_TYPE) : LH_SHORT_TYPE;
}

/* ---- the loop-carried words of the model, frame by frame; one wave per stream ----
 * Per frame: ath_adjust_factor before the frame's adjustment (lh_adjust_ATH on the loudness of the two granules the frame's
 * model hands on: the one before the frame and the frame's first), the masking adjustment the previous frame's CBR / ABR
 * loop leaves (by the block type of its last granule and channel: lh_encode_frame, reference quantize.c:1930-1940, 2029),
 * blocktype_old before either granule.  The wave takes 64 frames at a time: lane j reads frame j's few words, the
 * recurrence walks the 64 in order (every lane forms it, lane j keeps frame j's), lane j writes frame j's record -- the
 * chain waits for HBM once per 64 frames. */
#ifndef LH_EMU
extern "C" __global__ void __launch_bounds__(64)
#else
void
#endif
lh_ath_scan_kernel(const LhConfig * LH_KRESTRICT cfg, const LhTables * LH_KRESTRICT T, const LhStreamDesc * descs, const LhStreamState * states,
                   const LhMidFrame * frames, LhMidPsy * psy, int nstreams)
{
    int const sidx = (int) blockIdx.x;
    int const lane = (int) threadIdx.x;
    if (sidx >= nstreams)
        return;
    LhStreamDesc const d = lh_desc_uniform(descs, sidx);
    int const nf = d.frame_end - d.frame_begin;
    if (nf <= 0)
        return;
    const LhStreamState *st = &states[sidx];
    long long const base = d.out_index + d.mid_rel;
    int const two = lh_uni_i(cfg->channels == 2);
    float const mlow_long = lh_uni_f(cfg->masking_lower_long), mlow_short = lh_uni_f(cfg->masking_lower_short);
    float   factor = lh_uni_f(st->ath_adjust_factor), limit = lh_uni_f(st->ath_adjust_limit);
    float   before0 = lh_uni_f(st->loudness_sq_save[0]), before1 = lh_uni_f(st->loudness_sq_save[1]);
    float   mlow = lh_uni_f(st->masking_lower);
    int     bt0 = lh_uni_i(st->blocktype_old[0]), bt1 = lh_uni_i(st->blocktype_old[1]);
    for (int f0 = 0; f0 < nf; f0 += 64) {
        int const n = lh_uni_i(nf - f0 < 64 ? nf - f0 : 64);
        const LhMidSmall *ms = &frames[base + f0 + (lane < n ? lane : 0)].small;
        float const l00 = ms->gr[0].loud[0], l01 = ms->gr[0].loud[1], l10 = ms->gr[1].loud[0], l11 = ms->gr[1].loud[1];
        /* bits 0..3: uselong of (gr 0, ch 0), (gr 0, ch 1), (gr 1, ch 0), (gr 1, ch 1); bit 4: the frame's last granule and
         * channel is a short block */
        uint32_t const flags = (uint32_t) (ms->gr[0].uselong[0] != 0) | ((uint32_t) (ms->gr[0].uselong[1] != 0) << 1)
            | ((uint32_t) (ms->gr[1].uselong[0] != 0) << 2) | ((uint32_t) (ms->gr[1].uselong[1] != 0) << 3)
            | ((uint32_t) (ms->gr[1].block_type[two ? 1 : 0] == LH_SHORT_TYPE) << 4);
        float   my_factor = 0.0f, my_mlow = 0.0f;
        uint32_t my_bt = 0;
        for (int j = 0; j < n; j++) {
            float   loud[2][2];
            uint32_t const fl = lh_shfl_u32(flags, j);
            float const a00 = lh_shfl_f32(l00, j), a01 = lh_shfl_f32(l01, j), a10 = lh_shfl_f32(l10, j), a11 = lh_shfl_f32(l11, j);
            int const g1_0 = lh_blocktype_next(bt0, (int) (fl & 1u)), g1_1 = lh_blocktype_next(bt1, (int) ((fl >> 1) & 1u));
            if (lane == j) {
                my_factor = factor;
                my_mlow = mlow;
                my_bt = (uint32_t) bt0 | ((uint32_t) bt1 << 8) | ((uint32_t) g1_0 << 16) | ((uint32_t) g1_1 << 24);
            }
            bt0 = lh_blocktype_next(g1_0, (int) ((fl >> 2) & 1u));
            bt1 = lh_blocktype_next(g1_1, (int) ((fl >> 3) & 1u));
            /* one channel counts twice (reference encoder.c:72-79) */
            loud[0][0] = before0;
            loud[0][1] = two ? before1 : before0;
            loud[1][0] = a00;
            loud[1][1] = two ? a01 : a00;
            lh_adjust_ATH(T, loud, &factor, &limit);
            before0 = a10;
            before1 = a11;
            mlow = (fl & 16u) ? mlow_short : mlow_long;
        }
        if (lane < n) {
            LhMidPsy *pr = &psy[base + f0 + lane];
            pr->ath_factor = my_factor;
            pr->masking_lower = my_mlow;
            pr->bt_old[0][0] = (int8_t) (my_bt & 255u);
            pr->bt_old[0][1] = (int8_t) ((my_bt >> 8) & 255u);
            pr->bt_old[1][0] = (int8_t) ((my_bt >> 16) & 255u);
            pr->bt_old[1][1] = (int8_t) ((my_bt >> 24) & 255u);
            pr->pad = 0;
        }
    }
}

/* ---- stages 6 - 8 of every granule of the launch; one workgroup (wave w: pseudo-channels w and w + 2) per (stream, granule) ---- */
#ifndef LH_EMU
extern "C" __global__ void __launch_bounds__(LH_NT, 6)
#else
void
#endif
lh_psy_mask_kernel(const LhConfig * LH_KRESTRICT cfg, const LhTables * LH_KRESTRICT T, const LhStreamDesc * descs, const LhStreamState * states,
                   const LhMidFrame * frames, LhMidPsy * psy, int nstreams)
{
    LhLds & L = lh_lds;
    int const sidx = (int) blockIdx.y;
    LhCtx   c;
    c.cfg = cfg;
    c.T = T;
    c.st = nullptr;
    c.pcm = nullptr;
    c.pcmf = nullptr;
    c.d = lh_desc_uniform(descs, sidx);
    c.frame_base = 0;
    c.tid = (int) threadIdx.x;
    c.lane = c.tid & 63;
    c.wave = lh_uni_i(c.tid >> 6);
    int const g = (int) blockIdx.x;             /* the granule's place in the launch */
    if (g >= 2 * (c.d.frame_end - c.d.frame_begin))
        return;
    int const lane = c.lane, w = c.wave, gr = g & 1;
    int const n_chn_psy = (cfg->mode == LH_MODE_JOINT_STEREO) ? 4 : cfg->channels;
    long long const base = c.d.out_index + c.d.mid_rel;
    const LhMidFrame *rec = &frames[base + (g >> 1)];
    LhMidPsy *pr = &psy[base + (g >> 1)];
    const LhStreamState *st = &states[sidx];
    LhPsyCarry nb;
    /* the clamp's two previous long calls: the unclamped spread energies of granules g - 1 and g - 2, which for the launch's
     * first two granules are what the stream's previous launch left */
    for (int p = 0; p < 2; p++) {
        int const chn = w + 2 * p;
        nb.n1[p] = nb.n2[p] = 0.0f;
        if (chn < n_chn_psy) {
            nb.n1[p] = (g >= 1) ? frames[base + ((g - 1) >> 1)].lng.m[(g - 1) & 1][chn].v[1][lane] : st->nb_l1[chn][lane];
            nb.n2[p] = (g >= 2) ? frames[base + ((g - 2) >> 1)].lng.m[gr][chn].v[1][lane]
                : (g == 1) ? st->nb_l1[chn][lane] : st->nb_l2[chn][lane];
        }
    }
    if (c.tid < 2) {
        L.uselong[c.tid] = rec->small.gr[gr].uselong[c.tid];
        L.ss.blocktype_old[c.tid] = pr->bt_old[gr][c.tid];
    }
    else if (c.tid == 2)
        L.ss.masking_lower = pr->masking_lower;
    /* (the rows' last three words are padding: zero, so that the record is the same from run to run) */
    if (lane >= LH_XMIN_N)
        for (int p = 0; p < 2; p++)
            L.en[w + 2 * p][lane] = L.thm[w + 2 * p][lane] = 0.0f;
    float const ath_adjust_factor = lh_uni_f(pr->ath_factor);
    LH_SYNC_WG_LDS();
    LhPsyAt const at = { };
    lh_psy_stage_mask(c, gr, n_chn_psy, &rec->lng, nb, ath_adjust_factor, at);
    lh_psy_stage_bands(c, n_chn_psy, at);
    lh_psy_stage_short(c, gr, n_chn_psy, &rec->shrt, nb, ath_adjust_factor, at);
    /* (every stage ends with a workgroup barrier) */
    for (int p = 0; p < 2; p++) {
        int const chn = w + 2 * p;
        if (chn < n_chn_psy) {
            pr->en[gr][chn][lane] = L.en[chn][lane];
            pr->thm[gr][chn][lane] = L.thm[chn][lane];
        }
    }
}

#ifndef LH_EMU
/* both in order on the analysis kernels' HIP stream, behind lh_analysis_kernel (the scan reads the loudness it leaves) */
extern "C" int
lh_launch_psy_finish(const LhConfig * cfg, const LhTables * T, const LhStreamDesc * descs, const LhStreamState * states, LhMidPools mid,
                     LhMidPsy * psy, int nstreams, int max_frames, void *stream)
{
    if (nstreams <= 0 || max_frames <= 0)
        return 0;
    hipLaunchKernelGGL(lh_ath_scan_kernel, dim3((unsigned) nstreams), dim3(64), 0, (hipStream_t) stream, cfg, T, descs, states,
                       mid.frames, psy, nstreams);
    hipLaunchKernelGGL(lh_psy_mask_kernel, dim3((unsigned) (2 * max_frames), (unsigned) nstreams), dim3(LH_NT), 0, (hipStream_t) stream,
                       cfg, T, descs, states, mid.frames, psy, nstreams);
    return (int) hipGetLastError();
}
#else
extern "C" int
lh_emu_psy_finish(const LhConfig * cfg, const LhTables * T, const LhStreamDesc * descs, const LhStreamState * states,
                  const LhMidPools * pools, LhMidPsy * psy, int nstreams, int max_frames)
{
    LhMidPools const mid = *pools;
    hipemu_dim3 grid = { (unsigned) (2 * max_frames), (unsigned) nstreams, 1 }, b64 = { 64, 1, 1 }, b128 = { LH_NT, 1, 1 };
    hipemu_dim3 grid1 = { (unsigned) nstreams, 1, 1 };
    hipemu_run(grid1, b64,[=] () {
               lh_ath_scan_kernel(cfg, T, descs, states, mid.frames, psy, nstreams);
               }
    );
    hipemu_run(grid, b128,[=] () {
               lh_psy_mask_kernel(cfg, T, descs, states, mid.frames, psy, nstreams);
               }
    );
    return 0;
}
#endif
