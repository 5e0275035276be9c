/*
 * lh_lds_subband.h -- the LDS image of lh_subband.hip's workgroups (included by lh_dev_common.h in place of the encode
 * kernel's LhLds).  A wave (= channel) owns one plane of LH_SB_PLANE words and uses it three times per frame: as the
 * polyphase window of the frame, then -- the tap sums wait in registers until the wave has read the last sample -- as the
 * sub-band samples of the frame's two granules, then -- the MDCT's inputs wait in registers likewise -- as the spectra
 * that go to HBM.  The granule before the frame, which the MDCT overlaps with, has a place of its own (prev), written by
 * the lanes that read it as a frame's second granule.  Nothing of a channel is touched by the other wave.
 */
#define LH_SB_WIN 1632          /* the samples the 36 slots of a frame read: 286 + 32 * 35 + 224 + 1, rounded up to the swizzle's block */
#define LH_SB_HALF (LH_SB_WIN / 2)      /* words between the two granules' sub-band samples: >= LH_SB_GRANULE, a multiple of four */
#define LH_SB_PLANE (2 * LH_SB_HALF)
struct LhSbLds {
    float   sb[2][2][LH_SB_HALF];       /* [ch][granule of the frame][slot * LH_SB_STRIDE + band] (lh_subband_network) */
};
struct LhLds {
    float   mwin[4 * 36];       /* the MDCT windows and rotation constants (lh_mdct_win) */
    float   enw[288];           /* the polyphase window's coefficients (lh_enwindow), read a row per lane by the tap sums */
    float   prev[2][LH_SB_GRANULE];     /* [ch][slot * LH_SB_STRIDE + band]: the sub-band samples of the granule before the frame */
    union __attribute__((aligned(16))) {
        float   mf[2][LH_SB_PLANE];     /* (swizzled: LH_MF_SWZ) */
        float   xr[2][LH_SB_PLANE];     /* [ch][gr * 576 + line] */
        struct {
            LhSbLds mdct;
        } u;
        /* (named by lh_dev_common.h's helpers of the encode kernel, which this kernel does not call) */
        struct {
            LhCtxShared ctx;
            LhRgSlot rg[2];
        };
    };
};
static_assert(LH_SB_WIN % 32 == 0 && LH_SB_WIN <= LH_SB_PLANE && LH_SB_GRANULE <= LH_SB_HALF && 2 * 576 <= LH_SB_PLANE, "what a plane holds");
static_assert(LH_SB_HALF % 4 == 0, "the planes start on 16 bytes: the spectra leave as four-word vectors");
/* the budget: eight workgroups (four waves per SIMD, which is what the registers allow: lh_subband.hip) share a CU's 160 KB */
static_assert(sizeof(LhLds) <= 20480, "LDS budget of the sub-band kernel");
__shared__ LhLds lh_lds __attribute__((aligned(16)));
