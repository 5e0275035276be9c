/*
 * lh_lds_psyfin.h -- the LDS image of lh_psy_finish.hip's workgroups (included by lh_dev_common.h in place of the encode
 * kernel's LhLds): the partition arrays of one granule's four pseudo-channels and the band images made from them, 4.6 KB.
 */
struct LhLds {
    LhSmallState ss;            /* masking_lower and blocktype_old: read by lh_masking_tail, set per granule from the record */
    LhCtxShared ctx;
    LhRgSlot rg[2];
    int     uselong[2];
    int     pad[2];
    float   eb[4 * 64] __attribute__((aligned(16)));
    float   thr[4 * 64];
    float   en[4][64];          /* 22 long bands, 13 x 3 short ones (LhMidPsy's rows) */
    float   thm[4][64];
};
__shared__ LhLds lh_lds __attribute__((aligned(16)));
