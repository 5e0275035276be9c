/*
 * lh_api_int.h -- what the two halves of the C-ABI layer share: lh_api.cpp (the lame_* handle API) and lh_batch.cpp
 * (the lamehip_batch_* API).  Internal; nothing here is exported from the library.
 */
#ifndef LH_API_INT_H
#define LH_API_INT_H

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <mutex>

#include "lamehip.h"
#include "lamehip_types.h"
#include "lh_host.h"
#include "lh_device.h"
#include "lh_hip_own.h"
#include "lh_stats.h"

extern "C" int lh_launch_encode(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf,
                                const LhStreamDesc * descs, LhStreamState * states,
                                LhFrameOut * out, uint8_t * bytes, int nstreams, void *stream);

/* the same kernel compiled for MPEG-2 / 2.5 streams (lh_kernels.hip with -DLH_LSF: one granule per frame) */
extern "C" int lh_launch_encode_lsf(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf,
                                    const LhStreamDesc * descs, LhStreamState * states,
                                    LhFrameOut * out, uint8_t * bytes, int nstreams, void *stream);

/* the MPEG-1 kernel once more, compiled for the new VBR loop (lh_kernels.hip with -DLH_VBRK: same source, the
 * instruction scheduling strategy that loop runs best with; csrc/Makefile) */
extern "C" int lh_launch_encode_vbr(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf,
                                    const LhStreamDesc * descs, LhStreamState * states,
                                    LhFrameOut * out, uint8_t * bytes, int nstreams, void *stream);

/* the split pipeline: the analysis kernels (lh_analysis.hip, lh_subband.hip), which do everything of a
 * frame that depends on the PCM alone for all frames of a launch at once, and the encode kernels compiled to start from
 * their output (lh_kernels.hip with -DLH_SPLIT); one set per frame geometry / scheduling variant as above */
#define LH_DECL_SPLIT(sfx) \
    extern "C" int lh_launch_analysis##sfx(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf, \
                                           const LhStreamDesc * descs, const LhStreamState * states, LhMidPools mid, \
                                           int nstreams, int max_frames, void *stream); \
    extern "C" int lh_launch_subband##sfx(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf, \
                                          const LhStreamDesc * descs, LhStreamState * states, LhMidPools mid, \
                                          int nstreams, int max_frames, void *stream);
LH_DECL_SPLIT()
/* the front masking kernels of a CBR / ABR launch (lh_psy_finish.hip; MPEG-1 streams), behind the analysis kernels */
extern "C" int lh_launch_psy_finish(const LhConfig * cfg, const LhTables * T, const LhStreamDesc * descs, const LhStreamState * states,
                                    LhMidPools mid, LhMidPsy * psy, int nstreams, int max_frames, void *stream);
LH_DECL_SPLIT(_lsf)
#define LH_DECL_Q(sfx) \
    extern "C" int lh_launch_encode_q##sfx(const LhConfig * cfg, const LhTables * T, const int16_t * pcm, const float *pcmf, \
                                           const LhStreamDesc * descs, LhStreamState * states, LhFrameOut * out, \
                                           uint8_t * bytes, int nstreams, void *stream, LhMidPools mid, \
                                           const LhMidPsy * psy);
LH_DECL_Q()
LH_DECL_Q(_vbr)
LH_DECL_Q(_lsf)

extern "C" int lh_launch_selftest(unsigned *d_out, unsigned seed, void *stream);
extern "C" int lh_launch_summary(const LhStreamState * states, long long *sum, int nstreams, void *stream);
extern "C" int lh_launch_scatter(const int16_t * arena, int16_t * pool, long cap, const int *seg, int nseg, void *stream);
extern "C" int lh_launch_resample(const LhRsParams * p, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails,
                                  const LhRsStream * streams, int nstreams, int max_blocks, const int16_t * pcm, float *pcmf,
                                  void *stream);

#define LAME_ID 0xFFF88E3Bu     /* reference util.h:482 */

/* what lamehip_last_error() returns: one buffer per thread, defined in lh_api.cpp.  (__thread, not thread_local: a
 * thread_local declared in one file and defined in another is reached through an initialisation hook that this one, a
 * plain array, does not have -- and that a hidden weak reference in a shared library does not resolve to "none".) */
extern __thread char g_err[512] __attribute__((visibility("hidden")));

static inline int
set_err(const char *what, hipError_t e)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return LAMEHIP_ERR_DEVICE;
}

#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return set_err(#call, e_); } while (0)

/* samples per frame (1152; 576 for MPEG-2 / 2.5: one granule) and the samples that have to be buffered before a frame can
 * be encoded (BLKSIZE + framesize - FFTOFFSET: 1904 / 1328; reference lame.c:1627-1648) */
static inline int
fs_of(const LhConfig & c)
{
    return 576 * c.mode_gr;
}

static inline int
mfn_of(const LhConfig & c)
{
    return LH_BLKSIZE + 576 * c.mode_gr - LH_FFTOFFSET;
}

/* per device: the end of the last launch that filled it (lamehip_batch_encode) */
struct LhLaunchSerial {
    std::mutex lock;
    hipEvent_t ev = nullptr;
};

/* device-resident constants shared by a handle or a batch */
struct LhDeviceConst {
    LhConfig *d_cfg = nullptr;
    LhTables *d_tab = nullptr;
    int     lsf = 0;            /* an MPEG-2 / 2.5 stream: the kernel object compiled for one granule per frame */
    int     vbrk = 0;           /* an MPEG-1 stream in the new VBR loop: the object scheduled for that loop */
    int     front = 0;          /* an MPEG-1 stream in the CBR or ABR loop: its split launches run the front masking kernels */
    int front_psy() const { return front; }
    int launch(const int16_t * pcm, const float *pcmf, const LhStreamDesc * descs, LhStreamState * states,
               LhFrameOut * out, uint8_t * bytes, int nstreams, void *stream) const {
        return (lsf ? lh_launch_encode_lsf : vbrk ? lh_launch_encode_vbr : lh_launch_encode)
            (d_cfg, d_tab, pcm, pcmf, descs, states, out, bytes, nstreams, stream);
    }
    /* The split pipeline: analysis kernels for every frame of the launch, then the encode kernel that starts from what they
     * left in `mid'.  ev[0..1], when given, are recorded behind the analysis and the sub-band kernels (per-kernel times).  psy,
     * when not null (front_psy() says whether a launch may have one): the front masking kernels run behind the analysis kernels
     * -- their time counts as analysis -- and the encode kernel starts from their records. */
    int launch_split(const int16_t * pcm, const float *pcmf, const LhStreamDesc * descs, LhStreamState * states,
                     LhFrameOut * out, uint8_t * bytes, int nstreams, int max_frames, const LhMidPools & mid, LhMidPsy * psy, void *stream,
                     hipEvent_t * ev) const {
        int     rc;
        rc = (lsf ? lh_launch_analysis_lsf : lh_launch_analysis) (d_cfg, d_tab, pcm, pcmf, descs, states, mid, nstreams, max_frames, stream);
        if (rc)
            return rc;
        if (psy) {
            rc = lh_launch_psy_finish(d_cfg, d_tab, descs, states, mid, psy, nstreams, max_frames, stream);
            if (rc)
                return rc;
        }
        if (ev) {
            hipError_t const e = hipEventRecord(ev[0], (hipStream_t) stream);
            if (e != hipSuccess)
                return (int) e;
        }
        rc = (lsf ? lh_launch_subband_lsf : lh_launch_subband) (d_cfg, d_tab, pcm, pcmf, descs, states, mid, nstreams, max_frames, stream);
        if (rc)
            return rc;
        if (ev) {
            hipError_t const e = hipEventRecord(ev[1], (hipStream_t) stream);
            if (e != hipSuccess)
                return (int) e;
        }
        return (lsf ? lh_launch_encode_q_lsf : vbrk ? lh_launch_encode_q_vbr : lh_launch_encode_q)
            (d_cfg, d_tab, pcm, pcmf, descs, states, out, bytes, nstreams, stream, mid, psy);
    }
    int upload(const LhConfig & cfg, const LhTables & tab) {
        lsf = (cfg.mode_gr == 1);
        vbrk = !lsf && (cfg.vbr == 1 || cfg.vbr == 4);
        front = !lsf && (cfg.vbr == 0 || cfg.vbr == 3);
        HIPCHK(hipMalloc((void **) &d_cfg, sizeof(LhConfig)));
        HIPCHK(hipMalloc((void **) &d_tab, sizeof(LhTables)));
        HIPCHK(hipMemcpy(d_cfg, &cfg, sizeof(LhConfig), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_tab, &tab, sizeof(LhTables), hipMemcpyHostToDevice));
        return 0;
    }
    void release() {
        if (d_cfg)
            (void) hipFree(d_cfg);
        if (d_tab)
            (void) hipFree(d_tab);
        d_cfg = nullptr;
        d_tab = nullptr;
    }
};

/* Every handle and batch belongs to one HIP device: the one that was current when it was set up, or
 * the one named by lamehip_set_device / lamehip_batch_create_on.  Entry points that touch the device
 * make it current for the duration of the call and put the caller's device back afterwards. */
struct LhDeviceScope {
    int     prev = -1, mine = -1;
    explicit LhDeviceScope(int dev) {
        if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev && hipSetDevice(dev) == hipSuccess)
            mine = dev;
    }
    ~LhDeviceScope() {
        if (mine >= 0)
            (void) hipSetDevice(prev);
    }
};

/* (made by lame_init with `new lame_global_struct()': what has no initialiser below starts zeroed) */
struct lame_global_struct {
    unsigned class_id = LAME_ID;
    int     device = -1;        /* -1 until lame_init_params or lamehip_set_device fixes it */
    int     init_rc = 0;        /* what lame_init_params returned */
    /* message callbacks (reference lame.h:346-348, util.c:707-760): errors of this library's calls on the
     * handle go to report_err; nullptr silences them */
    lame_report_function report_err = nullptr, report_dbg = nullptr, report_msg = nullptr;
    LhUserParams p;
    int     out_samplerate = 0;
    int     write_vbr_tag = 1;  /* reference default (lame.c:2340) */
    int     inited = 0;
    int     have_device = 0;
    LhConfig cfg;
    LhTables *tab = nullptr;    /* host copy */
    LhDeviceConst dc;
    /* streaming state of the single-handle path */
    std::vector < float >hl, hr; /* transformed samples [hist_base, fed) kept on the host (in_buffer_0/1) */
    long long hist_base = 0;
    long long fed = 0;
    int     frames_done = 0;
    int     flushed = 0;
    LhDevBuf < LhStreamState > d_state;
    LhDevBuf < float >d_pcm;    /* two planes of cap() / 2 samples */
    LhDevBuf < LhStreamDesc > d_desc;
    LhDevBuf < LhFrameOut > d_out;
    std::vector < LhFrameOut > h_out;
    LhFrameOut last_frame;
    int     have_last = 0;
    LhBitstream bs = {};
    LhStream stream;
    int     nogap_total = 0, nogap_current = 0; /* the frontend's --nogap bookkeeping (lame_set_nogap_*) */
    int     find_replaygain = 0;        /* lame_set_findReplayGain: the title's radio gain goes into the LAME tag */
    LhReplayGain *rg = nullptr;
    /* Xing/Info + LAME tag (host bookkeeping, lh_vbrtag.c) */
    LhVbrTag tag = {};
    int     tag_placeholder_pending = 0;
    int     enc_padding = 0;
    /* input rate != output rate: the transformed samples pass through this first (lh_resample.c) */
    LhResampler *rs = nullptr;
    std::vector < float >tl, tr;
    /* what the frontend's progress display asks for (reference encoder.c:156-184 updateStats) */
    unsigned long num_samples = 0xFFFFFFFFul;   /* MAX_U_32_NUM, reference lame.c:2336 */
    int     preset_vbr = 0;     /* lame_set_preset chose a V0..V9 preset */
    int     frame_num_base = 0; /* frames before the last lame_init_bitstream */
    LhStatCarry hist = {};      /* mode[bitrate index | 15 = all][mode extension | 4 = frames], block[..][block type, 4 = mixed | 5 = granules] */
    /* (out of line now that the owners make it more than nothing; not a symbol of the library) */
    __attribute__((visibility("hidden"))) ~lame_global_struct() = default;
};

static inline int
valid(const lame_t g)
{
    return g && g->class_id == LAME_ID;
}

#endif /* LH_API_INT_H */
