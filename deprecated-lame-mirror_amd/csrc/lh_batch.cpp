/*
 * lh_batch.cpp -- the lamehip_batch_* API of liblamehip (declared in include/lamehip.h): many streams with one
 * set of settings, encoded by one launch of the split pipeline (or of the fused kernel).
 *
 * Host side only, like lh_api.cpp, which holds the lame_* handle API; what the two share is in lh_api_int.h.
 */
#include <time.h>
#include <thread>
#include <atomic>

#include "lh_api_int.h"
#include "lh_stats.h"
#include "lh_pcm_in.h"
#include "lh_gain.h"
#include "lh_replaygain_tables.h"
#include "lh_drain.h"

extern "C" int lh_launch_resample_typed(int type, const LhRsParams * p, const float *bank, const LhRsBlock * trunk, const LhRsBlock * tails,
                                        const LhRsStream * streams, int nstreams, int max_blocks, const void *pcm, float *pcmf,
                                        void *stream);
extern "C" int lh_launch_ingest(int type, const LhInParams * p, const LhInStream * streams, int nstreams, long long max_n, const void *in,
                                float *out, void *stream);
extern "C" int lh_launch_append(int type, const LhInParams * p, const LhApSeg * segs, int nsegs, long long max_n, void *pool, void *stream);
extern "C" int lh_launch_append_raw(int esz, const LhInParams * p, const LhApSeg * segs, int nsegs, long long max_n, void *pool, void *stream);
extern "C" int lh_launch_resample_tiles(int type, const LhRsParams * p, const float *bank, const LhRsTile * tiles, long long ntiles,
                                        const long long *lens, const void *pcm, float *pcmf, void *stream);
extern "C" int lh_launch_resample_mixed_tiles(int type, const LhRsParams * p, const LhRsClass * classes, int nclasses, const float *banks,
                                              const LhRsTile * tiles, long long ntiles, const long long *lens, const void *pcm, float *pcmf,
                                              void *stream);
extern "C" int lh_launch_deinterleave(int esz, const void *src_l, const void *src_r, void *dst_l, void *dst_r, long long n, void *stream);
extern "C" int lh_launch_gain(int floats, const LhGainParams * p, const LhGainStream * streams, int nstreams, const int *trunk, const int *tails,
                              const void *pool, double *pairs, void *stream);
extern "C" int lh_launch_gain_resume(int floats, const LhGainParams * p, const LhGainStream * streams, int nstreams, const int *tails,
                                     const void *pool, double *pairs, LhGainCarry * carry, void *stream);
extern "C" void lh_pcm_copy_plane(void *dst, const void *src, int esz, int stride, long n);
extern "C" int lh_launch_tag(const LhTagParams * p, const LhStreamDesc * descs, const LhStreamState * states, const LhFrameOut * out,
                             unsigned char *bytes, const unsigned char *tmpl, const int *padding, int nstreams, void *stream);
extern "C" int lh_launch_drain(const LhDrainParams * p, const LhStreamDesc * descs, const LhStreamState * states, const long long *drained,
                               long long *carry, const unsigned char *pool, LhDrainRow * rows, int nstreams, const LhDrainTile * tiles,
                               long long ntiles, unsigned char *round, long long round_cap, void *stream);
extern "C" int lh_launch_tag_resume(const LhTagParams * p, const LhTagPow * pw, const LhStreamDesc * descs, const LhStreamState * states,
                                    const LhDrainRow * rows, const LhFrameOut * out, const unsigned char *pool, const unsigned char *tmpl,
                                    const int *padding, LhTagCarry * carry, unsigned char *tags, int final, int nstreams, void *stream);
extern "C" int lh_launch_stats(const LhStreamDesc * descs, const LhFrameOut * out, int nstreams, int channels, int mode_gr, LhStatCarry * carry,
                               void *stream);
extern "C" int lh_launch_slot_restart(const int *list, int nlist, int nstreams, LhStreamState * states, const LhStreamState * states0,
                                      long long *drain_carry, LhTagCarry * tag_carry, LhGainCarry * gain_carry, void *stream);

/* per device: the end of the last launch that filled it (lamehip_batch_encode) */
static LhLaunchSerial &
launch_serial(int device)
{
    static LhLaunchSerial per_device[64];
    return per_device[(device >= 0 && device < 64) ? device : 0];
}

/* ====================================================================== */
/* batch extension                                                          */

/* Batches go through the split pipeline unless LAMEHIP_FUSED=1 asks for the single fused kernel (A/B measurements; the
 * handle API always uses the fused kernel: one frame per launch has nothing to analyse ahead). */
static int
batch_use_split(void)
{
    const char *e = getenv("LAMEHIP_FUSED");
    return !(e && e[0] == '1');
}

/* LAMEHIP_SPLIT_DENY=1, looked at before every launch: this launch takes the fused kernel as if the pools could not be had
 * (test aid: a batch whose launches change kernels mid-stream, tests/test_gpu_parity.py) */
static int
batch_split_denied(void)
{
    const char *e = getenv("LAMEHIP_SPLIT_DENY");
    return e && e[0] == '1';
}


/* (made by lamehip_batch_create_on with `new lamehip_batch()': what has no initialiser below starts zeroed or empty.
 * Everything HIP is held by an owner, lh_hip_own.h, and goes with `delete' -- inside the batch's LhDeviceScope.) */
struct lamehip_batch {
    int     device = 0;
    LhConfig cfg;
    LhTables *tab = nullptr;
    LhDeviceConst dc;
    int     B = 0;
    long    cap = 0;
    LhDevBuf < int16_t > d_pcm; /* [B][2][cap] elements of esz bytes (held in units of two bytes) */
    /* the sample type of the input pool and of its pinned mirror (lamehip_batch_set_sample_type): other than s16 the pool
     * holds int32 or float, the kernels read the float pool d_pcmf ([B][2][cap] when the batch does not convert the rate),
     * and lamehip_batch_encode fills that from the pool with lh_ingest.hip -- or with the rate converter, which then reads
     * the typed pool -- for the streams declared since their last ingest */
    int     stype = LH_PCM_S16;
    int     esz = 2;
    std::vector < char >in_dirty;
    std::vector < LhInStream > h_in_streams;
    LhDevBuf < LhInStream > d_in_streams;
    LhEvent ev_in[2];
    int     in_ran = 0;         /* the last lamehip_batch_encode ingested something (between ev_in[0] and ev_in[1]) */
    float   in_ms = 0;
    LhDevBuf < LhStreamState > d_state;
    LhDevBuf < LhStreamState > d_state0;        /* the streams' initial states (batch_reset_states) */
    LhDevBuf < LhStreamDesc > d_desc;
    LhDevBuf < LhFrameOut > d_out;
    std::vector < long >len;
    std::vector < int >nframes;
    std::vector < long long >out_off;
    /* device bit packing (lamehip_batch_set_device_packing) */
    int     dev_pack = 0;
    LhDevBuf < uint8_t > d_bytes;
    std::vector < long long >bytes_off;
    std::vector < LhStreamDesc > h_desc;
    /* device tagging on top of it (lamehip_batch_set_device_tagging): every stream's slice of the byte pool starts with room
     * for the Xing/Info + LAME tag frame (bytes_off[] and LhStreamDesc.bytes_base point behind it: the encode kernel, its
     * packer and the audio getters see what they always saw), lh_tag.hip fills the room behind the encode kernel from the
     * template the switch made, and the fetch brings whole file images home.  The radio gain, which becomes a number on the
     * host, is patched into an image when it is handed out. */
    int     dev_tag = 0;
    int     tagged = 0;         /* the last lamehip_batch_encode ran with the switch on ... */
    int     tag_room = 0;       /* ... and left this much room in front of every stream's audio (0: the tag does not fit a frame) */
    LhTagParams tag_p = {};
    LhDevBuf < unsigned char >d_tag_tmpl;
    LhDevBuf < int >d_tag_pad;
    std::vector < int >h_tag_pad;       /* the end padding per stream, as the last launch's kernel read it */
    std::vector < char >tag_patched;    /* stream s's image in h_bytes carries its gain */
    LhEvent ev_tag[2];
    int     tag_ran = 0;        /* the last lamehip_batch_encode launched the tag kernel (between ev_tag[0] and ev_tag[1]) */
    float   tag_ms = 0;
    LhStream stream;
    LhEvent ev0, ev1;
    float   last_ms = 0;
    int     encoded = 0;
    /* input rate != output rate: set_pcm converts on the host (as the reference's frontend would have
     * it: lame_encode_buffer calls of 1152 input samples, then the flush) into a float pool */
    int     rate_in = 0;
    LhResampler *rs = nullptr;
    LhDevBuf < float >d_pcmf;   /* [B][2][capf] */
    long    capf = 0;
    std::vector < int >padding; /* encoder_padding per stream (tag frame) */
    /* ... or, after lamehip_batch_set_device_resampling, on the device: the s16 pool d_pcm holds the input ([B][2][cap] at
     * the input rate, with its pinned mirror and device-side entry points as in a batch that does not convert), the host
     * only plans (lh_rs_trunk_extend / lh_rs_plan_tail: the blocks all streams share, and each stream's own last blocks) and
     * lamehip_batch_encode launches lh_resample_dev.hip over the streams declared since their last conversion */
    int     dev_rs = 0;
    int     pcm_given = 0;      /* PCM (or a length, or the mirror) has been handed over: the converter's place is settled */
    LhRsTrunk trunk = {};
    std::vector < long >len_in; /* input samples per stream (len[] is the converted length) */
    std::vector < std::vector < LhRsBlock > >tail;
    std::vector < char >rs_dirty;       /* declared since the stream's last conversion */
    std::vector < LhRsBlock > h_tails;  /* what the last launch's plan consisted of besides the trunk */
    std::vector < LhRsStream > h_rs_streams;
    LhDevBuf < float >d_rs_bank;
    LhDevBuf < LhRsBlock > d_rs_trunk, d_rs_tails;
    LhDevBuf < LhRsStream > d_rs_streams;
    long    rs_trunk_up = 0;    /* blocks of the trunk uploaded so far */
    LhEvent ev_rs[2];
    int     rs_ran = 0;         /* the last lamehip_batch_encode converted something (between ev_rs[0] and ev_rs[1]) */
    float   rs_ms = 0;
    /* ... or, after lamehip_batch_set_incremental_resampling on top of that, round by round: the appends put their chunks
     * into the input pool as they are and plan their calls at once (lh_rs_plan_call from the stream's cursor, cut into
     * tiles), lamehip_batch_encode_available / _finish run ONE launch of lh_resample_tiles_kernel over the tiles planned
     * since the last round, between the append launches and the encode launch -- a chunk's first outputs reach back into
     * the chunk before, which may still be in the staging arena when the append returns */
    int     inc_rs = 0;
    long    inc_capf = 0;       /* converted samples per stream the appends allow: capf (less under LAMEHIP_INC_RS_ROOM) */
    std::vector < LhRsCursor > rs_cur;  /* per stream: the converter behind the calls so far */
    std::vector < long long >rs_conv;   /* per stream: converted samples the rounds so far have put into the float pool */
    std::vector < LhRsBlock > rs_blk;   /* the blocks of the call being planned */
    std::vector < LhRsTile > h_tiles;   /* the round's tiles */
    std::vector < long long >h_rs_lens; /* input samples per stream, as the round's launch sees them */
    LhDevBuf < LhRsTile > d_tiles;
    LhDevBuf < long long >d_rs_lens;
    /* ... with streams at input rates of their own (lamehip_batch_set_stream_in_samplerate): every distinct rate is a CLASS
     * -- a converter for the plans, made on first use and kept until the batch goes; class 0 is the batch's own rate, `rs' --,
     * a stream's appends and flush are planned with its class's converter and its tiles carry the class, and a round in which
     * a stream has a class other than 0 is converted by ONE launch of lh_resample_mixed_tiles_kernel, which reads the class
     * table and all banks from HBM.  Nothing of this exists in a batch that never makes the call. */
    LhUserParams user_p;        /* the handle's settings: a new rate is accepted when they resolve to this batch's records with it */
    int     rs_ncls = 0;        /* classes made (0: the call was never accepted for another rate than the batch's) */
    LhResampler *rs_cls[LH_RS_CLASSES_MAX] = { };       /* [0] is `rs'; the others are the batch's to free */
    LhRsClass h_rs_cls[LH_RS_CLASSES_MAX] = { };
    std::vector < int >rs_scls; /* per stream: its class (empty until the first class is made) */
    LhDevBuf < float >d_rs_banks;       /* LH_RS_CLASSES_MAX banks of 2 * LH_RS_MAXPHASES + 1 rows of LH_RS_ROW floats */
    LhDevBuf < LhRsClass > d_rs_classes;
    /* ReplayGain (lamehip_batch_set_replaygain): lamehip_batch_encode measures the radio gain of the streams declared since
     * their last analysis with lh_gain.hip, behind the conversion / ingest kernels and in front of the analysis kernels.  The
     * host plans (lh_gain_plan: the blocks the handle API would hand to lh_rg_block), the kernel leaves every stream's window
     * sums in rg_pairs, and the first getter brings them to rg_win, where bins and gain are made of them (lh_replaygain.c). */
    int     rg_on = 0;
    int     rg_measured = 0;    /* an encode with the switch on has run since the last reset */
    int     rg_pending = 0;     /* the last launch's window sums are still on the device */
    std::vector < char >rg_dirty;       /* declared since the stream's last analysis */
    std::vector < long >rg_len_in;      /* a batch that converts on the host: input samples behind len[] */
    std::vector < std::vector < double > >rg_win;       /* per stream: (lsum, rsum) per finished window */
    std::vector < int >rg_tenths;
    std::vector < LhGainStream > h_rg_streams;
    std::vector < int >h_rg_tails, h_rg_trunk;
    LhDevBuf < LhGainStream > d_rg_streams;
    LhDevBuf < int >d_rg_tails, d_rg_trunk;
    LhDevBuf < double >d_rg_pairs;
    LhEvent ev_rg[2];
    int     rg_ran = 0;         /* the last lamehip_batch_encode analysed something (between ev_rg[0] and ev_rg[1]) */
    float   rg_ms = 0;
    /* ... or, after lamehip_batch_set_incremental_replaygain, round by round once the batch is fed with appends: every append
     * is planned at once as the call to the analysis it is (lh_gain_plan_call from the stream's cursor; a batch that converts:
     * the made counts of the conversion's call plan), lamehip_batch_encode_available / _finish run ONE launch of
     * lh_gain_resume_kernel over the blocks planned since the last round, behind the append and conversion launches, and the
     * round's window sums come home with the round's wait.  What a stream carries between rounds stays in HBM (LhGainCarry). */
    int     inc_rg = 0;
    int     rg_was_on = 0;      /* rg_on as it was before the switch (which sets it: until the first append whole streams are measured) */
    int     rg_closed = 0;      /* lamehip_batch_finish has analysed the flush: the gains are final */
    long long inc_rg_max = 0;   /* samples of a stream the analysis takes: LH_GN_MAX_TOTAL (less under LAMEHIP_INC_RG_MAX) */
    std::vector < LhGainCursor > rg_cur;        /* per stream: the analysis behind the calls so far (a batch that converts: rs_cur) */
    std::vector < std::vector < int > >rg_blk;  /* per stream: the blocks planned since the last round */
    std::vector < long long >rg_heard;  /* per stream: samples the rounds so far have analysed (the carry's `heard') */
    std::vector < double >h_rg_round;   /* the round's window sums, on their way home */
    LhDevBuf < LhGainCarry > d_rg_carry;
    /* incremental use (lamehip_batch_append ...): samples in the pool / frames encoded per stream, a
     * packer and the bytes not yet drained per stream, and the pinned staging area of the next
     * lamehip_batch_encode_available (see h_stage below) */
    int     incremental = 0;
    std::vector < long >fed;
    std::vector < int >done;
    std::vector < int >staged;
    std::vector < LhBitstream > packer;
    std::vector < std::vector < unsigned char > >pending;
    std::vector < LhFrameOut > last;
    std::vector < char >have_last;
    /* pinned / HBM: [B descriptors][LH_STAGE_SEGS x 4 ints: the chunks][arena of staged samples, back to back] */
    LhPinned < unsigned char >h_stage;
    LhDevBuf < unsigned char >d_stage;
    long    stage_arena_at = 0; /* byte offset of the arena */
    long    stage_cap = 0;      /* shorts the arena holds (a 4-byte element of lamehip_batch_append_input counts as two) */
    long    stage_used = 0;     /* shorts staged */
    int     stage_nseg = 0;     /* chunks staged by lamehip_batch_append */
    int     finished = 0;       /* lamehip_batch_finish has run: the streams are closed */
    /* ... as a pool of B slots (lamehip_batch_end_stream / _restart_stream): a stream ends alone, with the next round -- its
     * flush planned and encoded as lamehip_batch_finish does it for all of them, its gain and tag frame made --, while the
     * others go on, and its slot takes the next stream once its bytes have been handed out.  What the restarted slots keep
     * in HBM from round to round is put back by ONE launch of lh_slot_restart_kernel (lh_slots.hip) on the batch's stream,
     * at the head of the next round, between ev_sl[0] and ev_sl[1]. */
    std::vector < char >slot;   /* per stream: LH_SLOT_LIVE, _ENDING (lamehip_batch_end_stream: the next round flushes it), _ENDED */
    std::vector < char >ending; /* per stream: the round in progress flushes it */
    std::vector < char >rg_final;       /* per stream: its flush has been analysed, rg_tenths[] is its gain */
    std::vector < char >tg_has; /* per stream: h_tg_tags holds its final frame */
    LhPinned < unsigned char >h_tg_round;       /* [B][tg_p.total]: the frames of a round in which only some streams end, on their way */
    std::vector < int >sl_list, sl_sent;        /* slots restarted since the last round; the list the last restart launch was given */
    LhDevBuf < int >d_sl_list;
    LhEvent ev_sl[2];
    int     sl_ran = 0;         /* the restart launch ev_sl[] are around has not been timed yet */
    int     sl_gap = 0;         /* sl_ms is a launch of the gap in progress (lamehip_batch_get_state asked for it) */
    float   sl_ms = 0;
    /* ... on the device packer (lamehip_batch_set_incremental_packing on top of lamehip_batch_set_device_packing): every stream
     * has a fixed slice of the byte pool d_bytes, laid out at the first append from the batch's capacity -- the encode kernel
     * writes at absolute positions across the rounds --, no LhFrameOut comes home and no host packer runs; behind a round's
     * encode launch lh_drain.hip finds what every stream has finished and gathers it from `drained' on into d_round, and the
     * round's table and bytes come home to h_dr_rows / h_round, out of which lamehip_batch_drain / _drain_ptr hand them */
    int     inc_pack = 0;
    long long dr_slice = 0;     /* bytes of a stream's slice */
    int     dr_frame_max = 0;   /* the largest frame the settings allow */
    int     dr_have = 0;        /* h_dr_rows / h_round hold a round's drain */
    std::vector < long long >dr_drained;        /* per stream: bytes handed out so far */
    std::vector < long long >dr_sent;   /* ... as the round's launch sees them */
    std::vector < long long >dr_bound;  /* per stream: the most the round can find */
    std::vector < long long >dr_next;   /* per stream: where its frames ended when the last table came home */
    std::vector < int >dr_done;         /* ... and how many there were */
    std::vector < LhDrainTile > h_dr_tiles;
    long long dr_padded = 0;    /* bytes of a round buffer that holds every stream's bound */
    LhDevBuf < long long >d_dr_drained, d_dr_carry;
    LhDevBuf < LhDrainTile > d_dr_tiles;
    LhDevBuf < LhDrainRow > d_dr_rows;
    LhPinned < LhDrainRow > h_dr_rows;  /* [B + 1]; a stream's n goes to 0 when it is handed out */
    LhDevBuf < unsigned char >d_round;
    LhPinned < unsigned char >h_round;
    LhEvent ev_dr[2];
    int     dr_ran = 0;         /* the last round launched the drain kernels (between ev_dr[0] and ev_dr[1]) */
    float   dr_ms = 0;
    /* ... with tag frames (lamehip_batch_set_incremental_tagging): a carry per stream in HBM (lh_tag.h: LhTagCarry) that ONE
     * launch of lh_tag_resume_kernel moves on behind every round's drain -- the music CRC over the bytes that became final,
     * the seek table's bookkeeping over the round's records --; the final round's launch makes the frames of it, which come
     * home to h_tg_tags behind the table, out of which lamehip_batch_tag_ptr / _get_tags_all hand them */
    int     inc_tag = 0;
    int     tg_have = 0;        /* h_tg_tags holds the final round's frames (and h_dr_rows their streams' statuses) */
    LhTagParams tg_p = {};      /* (total 0: the tag does not fit a frame, nothing is launched) */
    LhDevBuf < LhTagCarry > d_tg_carry;
    LhDevBuf < LhTagPow > d_tg_pow;
    LhDevBuf < unsigned char >d_tg_tmpl, d_tg_tags;
    LhDevBuf < int >d_tg_pad;
    std::vector < int >h_tg_pad;        /* the end padding per stream, as the final round's kernel read it */
    LhPinned < unsigned char >h_tg_tags;        /* [B][tg_p.total] */
    std::vector < char >tg_patched;     /* stream s's frame in h_tg_tags carries its gain */
    LhEvent ev_tg[2];
    int     tg_ran = 0;         /* the last round launched the tag kernel (between ev_tg[0] and ev_tg[1]) */
    std::vector < std::vector < unsigned char > >handed;        /* host packer: what lamehip_batch_drain_ptr last handed out */
    /* typed and device-resident appends (lamehip_batch_append_input / _append_input_device / _append_device): the table of
     * segments lh_append_kernel works through, pinned and in HBM -- entries [0, LH_STAGE_SEGS) for the chunks staged in the
     * arena, the B behind them for a round that comes from device buffers --, and the events around its launches */
    LhPinned < LhApSeg > h_ap;
    LhDevBuf < LhApSeg > d_ap;
    int     ap_nseg = 0;        /* chunks staged by lamehip_batch_append_input */
    long long ap_max_n = 0;     /* the longest of them */
    LhEvent ev_ap[2];
    int     ap_timed = 0;       /* ev_ap[] are around a launch whose time is not part of ap_ms yet */
    float   ap_ms = 0;          /* append launches since, and including, the last lamehip_batch_encode_available / _finish */
    std::vector < LhFrameOut > h_new;
    /* pinned host side of a pipelined batch (lamehip_batch_pcm_host_ptr / _upload / _fetch): the mirror of the
     * s16 pool the caller (or lamehip_batch_set_pcm) writes, which reaches HBM with one asynchronous copy on
     * the batch's stream; the device packer's bytes and a two-word summary per stream (bytes, status) on the
     * way back.  Another batch's copies and kernel run meanwhile (each batch has its own stream). */
    LhPinned < int16_t > h_pcm;
    std::vector < char >row_dirty;      /* streams whose mirror rows are newer than the pool */
    int     n_dirty = 0;
    LhPinned < unsigned char >h_bytes;
    LhDevBuf < long long >d_sum;
    LhPinned < long long >h_sum;
    int     fetched = 0;        /* the bytes of the last encode are in (or on their way into) h_bytes */
    /* the copies of a pipelined batch have streams of their own (different hardware queues from the kernel's, and
     * from each other: an upload queued behind the previous round's download on one stream cost 12 % of the
     * pipeline's throughput), tied to the kernel's stream by events; made by batch_copy_streams, all five at once */
    LhStream up_stream, down_stream;
    LhEvent ev_up, ev_sum, ev_down;
    int     up_pending = 0, down_pending = 0;
    int     up_inflight = 0;    /* an H2D copy out of the pinned mirror may still be running (host view: cleared only after ev_up) */
    int     launched = 0;       /* a kernel was launched on this batch and ev1 recorded (survives lamehip_batch_reset) */
    /* the split pipeline's pool (one record per frame of a launch, like d_out) and the events between its kernels */
    LhDevBuf < LhMidFrame > mid;
    /* the front masking kernels' records beside them, same index and as many (a batch whose launches run them: CBR / ABR,
     * MPEG-1; LhDeviceConst::front_psy) */
    LhDevBuf < LhMidPsy > midpsy;
    int     split = 0;          /* this batch's launches go through the split pipeline (batch_use_split) */
    LhEvent ev_part[2];
    LhEvent ev_wait;            /* behind the launch; only ever polled (hipEventQuery between short sleeps in lamehip_batch_sync): the
                                 * host thread sleeps instead of spinning on the stream (a rank per GPU must not burn a CPU per rank
                                 * while its kernel runs) */
    float   part_ms[3] = { 0, 0, 0 };   /* analysis, sub-band, encode kernel of the last launch (0: fused launch) */
    int     last_split = 0;
    /* a launch in windows of frames (batch_plan): the windows' descriptors (host, then HBM: [window][stream]) and three events
     * per window (its start, behind its analysis kernels, behind its sub-band kernel) */
    std::vector < LhStreamDesc > h_wdesc;
    LhDevBuf < LhStreamDesc > d_wdesc;
    std::vector < LhEvent > ev_win;
    int     last_windows = 1;   /* sub-launches of the last launch (1: the whole launch at once) */
    /* statistics (lamehip_batch_set_statistics): a record per stream in HBM (lh_stats.h: LhStatCarry, the reference's two
     * tables) that ONE launch of lh_stats_resume_kernel moves on behind every encode launch, a one-shot batch's and a round's
     * alike, between ev_st[0] and ev_st[1] -- the launch's records are counted where they lie, none comes home for it.  The
     * getters fetch the whole array on first use after a launch and serve from h_st until the next one.  Nothing of this
     * exists in a batch without the switch. */
    int     st_on = 0;
    LhDevBuf < LhStatCarry > d_st_carry;
    std::vector < LhStatCarry > h_st;
    int     st_have = 0;        /* h_st is what d_st_carry holds */
    LhEvent ev_st[2];
    int     st_ran = 0;         /* the last launch was followed by the statistics kernel (between ev_st[0] and ev_st[1]) ... */
    int     st_timed = 0;       /* ... and st_ms is its time */
    float   st_ms = 0;
};

enum { LH_SLOT_LIVE = 0, LH_SLOT_ENDING = 1, LH_SLOT_ENDED = 2 };

/* what batch_plan decides about a launch (outside the devices' launch order: it may allocate) and batch_launch carries out */
struct LhLaunchPlan {
    long long total;            /* frames of the launch */
    int     max_frames;         /* of its longest stream */
    int     split;              /* the split pipeline (else the fused kernel) */
    int     window;             /* frames per stream and sub-launch; 0: the whole launch at once */
    int     nwin;
};

/* room for `need' records in the split pipeline's pool (0), or not (-1: the pool is gone, *free_records says how many would
 * fit and lamehip_last_error() why) */
static int
batch_mid_reserve(lamehip_batch * b, long long need, long long *free_records = nullptr)
{
    /* (the encode kernel touches the record BEHIND the one it works on, the launch's last frame included: one spare
     * record has to exist whatever the launch's total is -- a later launch whose total equals the capacity must not
     * read past the pool) */
    if (free_records)
        *free_records = 0;
    size_t const rec_b = sizeof(LhMidFrame) + (b->dc.front_psy() ? sizeof(LhMidPsy) : 0);      /* per frame, both pools */
    if (need + 1 <= (long long) b->mid.cap() && (!b->dc.front_psy() || b->midpsy.cap() == b->mid.cap()))
        return 0;
    size_t  free_b = 0, total_b = 0;
    long long const want = need + 64;
    /* (the old pools go first, unlike LhDevBuf::reserve: what they held counts as free for the new ones) */
    b->mid.release();
    b->midpsy.release();
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess)
        free_b = 0;
    {
        /* LAMEHIP_MID_BUDGET_MB=n: no more than n MB count as free (test aid: the window size as a device with little
         * memory left would choose it) */
        const char *e = getenv("LAMEHIP_MID_BUDGET_MB");
        long const mb = e ? strtol(e, nullptr, 10) : 0;
        if (mb > 0 && (size_t) mb * 1000000u < free_b)
            free_b = (size_t) mb * 1000000u;
    }
    if (free_records)
        *free_records = (long long) (0.8 * (double) free_b / (double) rec_b) - 64;
    if ((double) want * (double) rec_b > 0.8 * (double) free_b) {
        /* (not an error: the launch runs in windows or takes the fused kernel; lamehip_last_error() says why) */
        snprintf(g_err, sizeof(g_err), "split pipeline: %lld frames need %.1f GB of analysis records, %.1f GB free",
                 need, (double) want * (double) rec_b / 1e9, (double) free_b / 1e9);
        return -1;
    }
    if (b->mid.alloc((size_t) want) != hipSuccess || (b->dc.front_psy() && b->midpsy.alloc((size_t) want) != hipSuccess)) {
        (void) hipGetLastError();
        b->mid.release();
        snprintf(g_err, sizeof(g_err), "split pipeline: hipMalloc of %.1f GB of analysis records failed",
                 (double) want * (double) rec_b / 1e9);
        return -1;
    }
    return 0;
}

/* LAMEHIP_MID_WINDOW=n, looked at before every launch: the split pipeline works through a launch in windows of n frames per
 * stream whatever the memory would allow (tuning / test aid; 0 or unset: windows only when the records of the whole launch
 * do not fit) */
static int
batch_window_env(void)
{
    const char *e = getenv("LAMEHIP_MID_WINDOW");
    long const v = e ? strtol(e, nullptr, 10) : 0;
    return (v > 0 && v < (1l << 30)) ? (int) v : 0;
}

#define LH_MID_WINDOW_MIN 64    /* frames: below that the fused kernel is the better launch (a sub-launch ends with its slowest stream) */

/* records a launch in windows of w frames needs at once (every stream's first window is its largest) */
static long long
batch_window_records(const lamehip_batch * b, const LhStreamDesc * h_descs, int w)
{
    long long n = 0;
    for (int s = 0; s < b->B; s++) {
        int const nf = h_descs[s].frame_end - h_descs[s].frame_begin;
        if (nf > 0)
            n += nf < w ? nf : w;
    }
    return n;
}

/* What the launch of the frames `h_descs' names will be: the split pipeline over the whole launch when its analysis records
 * fit the device (34 KB per frame, 38 KB with the front masking kernels' records: 90 GB at 1024 x 60 s), else the split pipeline over windows of as many frames per stream as
 * do fit -- each window a launch of its own, analysis kernels then encode kernel, the streams' state carried in
 * LhStreamState as between two launches of an incremental batch --, else (under LH_MID_WINDOW_MIN frames per window, more
 * than 65 535 streams, LAMEHIP_FUSED / LAMEHIP_SPLIT_DENY) the fused kernel.  The windows' descriptors go to HBM here, on the
 * batch's stream.  Allocates: call it before the devices' launch order is taken. */
static int
batch_plan(lamehip_batch * b, const LhStreamDesc * h_descs, LhLaunchPlan * p)
{
    long long free_records = 0;
    int     nactive = 0;
    memset(p, 0, sizeof(*p));
    for (int s = 0; s < b->B; s++) {
        int const nf = h_descs[s].frame_end - h_descs[s].frame_begin;
        if (nf > 0) {
            p->total += nf;
            nactive++;
            if (nf > p->max_frames)
                p->max_frames = nf;
        }
    }
    p->nwin = 1;
    /* (the analysis and sub-band kernels index the stream by blockIdx.y, which ends at 65535: a larger batch keeps the
     * fused kernel, whose grid is one-dimensional) */
    if (!(b->split && p->total > 0 && b->B <= 65535 && !batch_split_denied()))
        return 0;
    int     w = batch_window_env();
    if (w >= p->max_frames)
        w = 0;
    if (w == 0) {
        if (batch_mid_reserve(b, p->total, &free_records) == 0) {
            p->split = 1;
            return 0;
        }
        w = nactive ? (int) (free_records / nactive < p->max_frames ? free_records / nactive : p->max_frames) : 0;
        if (w < LH_MID_WINDOW_MIN) {
            size_t const n = strlen(g_err);
            snprintf(g_err + n, sizeof(g_err) - n, ": fused kernel");
            return 0;
        }
    }
    if (batch_mid_reserve(b, batch_window_records(b, h_descs, w)) != 0)
        return 0;
    p->split = 1;
    p->window = w;
    p->nwin = (p->max_frames + w - 1) / w;
    /* window k of a stream: its frames [begin + k w, begin + (k + 1) w) at the payload's places, their records from the
     * start of the pool on, stream after stream; the flush goes with the stream's last frame (a stream without frames
     * keeps its descriptor in window 0: what an incremental batch's launch may hold) */
    b->h_wdesc.resize((size_t) p->nwin * (size_t) b->B);
    for (int k = 0; k < p->nwin; k++) {
        long long at = 0;
        for (int s = 0; s < b->B; s++) {
            LhStreamDesc d = h_descs[s];
            int const nf = d.frame_end > d.frame_begin ? d.frame_end - d.frame_begin : 0;
            long long const lo = (long long) k * w < nf ? (long long) k * w : nf, hi = lo + w < nf ? lo + w : nf;
            if (nf > 0) {
                d.out_index = h_descs[s].out_index + lo;
                d.frame_begin = h_descs[s].frame_begin + (int) lo;
                d.frame_end = h_descs[s].frame_begin + (int) hi;
                d.flush = h_descs[s].flush && hi == nf && lo < hi;
                d.mid_rel = (int) (at - d.out_index);
                at += hi - lo;
            }
            else if (k > 0)
                d.flush = 0;
            b->h_wdesc[(size_t) k * (size_t) b->B + (size_t) s] = d;
        }
    }
    HIPCHK(b->d_wdesc.reserve(b->h_wdesc.size()));
    HIPCHK(hipMemcpyAsync(b->d_wdesc.get(), b->h_wdesc.data(), b->h_wdesc.size() * sizeof(LhStreamDesc), hipMemcpyHostToDevice, b->stream));
    while (b->ev_win.size() < 3 * (size_t) p->nwin) {
        LhEvent e;
        if (e.create() != hipSuccess)
            return set_err("hipEventCreate", hipGetLastError());
        b->ev_win.push_back(std::move(e));
    }
    return 0;
}

/* one launch of the batch's frames [frame_begin, frame_end) per stream, as `descs' (device copy) / `h_descs' say, between
 * ev0 and ev1 on the batch's stream, the way batch_plan decided */
static int
batch_launch(lamehip_batch * b, const int16_t * pcm, const float *pcmf, const LhStreamDesc * descs, const LhLaunchPlan & p, uint8_t * bytes)
{
    int     rc = 0, split = p.split;
    void   *const stream = (void *) (hipStream_t) b->stream;
    LhMidPools const mid = { b->mid.get() };
    LhMidPsy *const psy = b->dc.front_psy() ? b->midpsy.get() : nullptr;    /* (as large as the frames' pool: batch_mid_reserve) */
    if (split && !p.window && !b->ev_part[0]) {
        if (b->ev_part[0].create() != hipSuccess || b->ev_part[1].create() != hipSuccess)
            return set_err("hipEventCreate", hipGetLastError());
    }
    HIPCHK(hipEventRecord(b->ev0, b->stream));
    if (split && p.window) {
        for (int k = 0; k < p.nwin && !rc; k++) {
            int const left = p.max_frames - k * p.window;
            hipEvent_t between[2] = { b->ev_win[3 * (size_t) k + 1], b->ev_win[3 * (size_t) k + 2] };
            HIPCHK(hipEventRecord(b->ev_win[3 * (size_t) k], b->stream));
            rc = b->dc.launch_split(pcm, pcmf, b->d_wdesc.get() + (size_t) k * (size_t) b->B, b->d_state.get(), b->d_out.get(), bytes,
                                    b->B, left < p.window ? left : p.window, mid, psy, stream, between);
        }
    }
    else if (split) {
        hipEvent_t between[2] = { b->ev_part[0], b->ev_part[1] };
        rc = b->dc.launch_split(pcm, pcmf, descs, b->d_state.get(), b->d_out.get(), bytes, b->B, p.max_frames, mid, psy, stream, between);
    }
    else
        rc = b->dc.launch(pcm, pcmf, descs, b->d_state.get(), b->d_out.get(), bytes, b->B, stream);
    if (rc)
        return set_err("kernel launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev1, b->stream));
    b->st_ran = b->st_timed = 0;
    b->st_ms = 0;
    if (b->st_on) {
        /* statistics: the launch's records into the streams' tables, behind the (last window's) encode kernel and outside
         * ev0 .. ev1; `descs' are the whole launch's whatever the windows, out_index the payload's */
        HIPCHK(hipEventRecord(b->ev_st[0], b->stream));
        rc = lh_launch_stats(descs, b->d_out.get(), b->B, b->cfg.channels, b->cfg.mode_gr, b->d_st_carry.get(), stream);
        if (rc)
            return set_err("statistics launch", (hipError_t) rc);
        HIPCHK(hipEventRecord(b->ev_st[1], b->stream));
        b->st_ran = 1;
        b->st_have = 0;
    }
    if (b->ev_wait.create(hipEventDisableTiming) != hipSuccess)
        (void) hipGetLastError();
    if (b->ev_wait)
        HIPCHK(hipEventRecord(b->ev_wait, b->stream));
    b->last_split = split;
    b->last_windows = (split && p.window) ? p.nwin : 1;
    return 0;
}

static int
batch_padding(const lamehip_batch * b, int s)
{
    return b->rate_in ? b->padding[(size_t) s] : lh_end_padding_fs(b->len[(size_t) s], fs_of(b->cfg));
}

/* the kernels of this batch read the float pool */
static int
batch_reads_floats(const lamehip_batch * b)
{
    return b->rate_in || b->stype != LH_PCM_S16;
}

/* the rate class of stream s, and the converter its calls are planned with */
static int
batch_stream_cls(const lamehip_batch * b, int s)
{
    return b->rs_scls.empty() ? 0 : b->rs_scls[(size_t) s];
}

static const LhResampler *
batch_stream_rs(const lamehip_batch * b, int s)
{
    return b->rs_scls.empty() ? b->rs : b->rs_cls[b->rs_scls[(size_t) s]];
}

/* a stream has an input rate other than the batch's (lamehip_batch_set_stream_in_samplerate) */
static int
batch_own_rates(const lamehip_batch * b)
{
    for (int c:b->rs_scls)
        if (c != 0)
            return 1;
    return 0;
}

/* what the whole-stream calls say to a batch with such a stream: the one-shot converter shares one trunk of blocks between
 * all streams and stays single-rate.  Returns 0 when there is none */
static int
batch_refuse_own_rates(const lamehip_batch * b, const char *who)
{
    if (!b || !batch_own_rates(b))
        return 0;
    snprintf(g_err, sizeof(g_err), "%s: a stream of this batch has an input rate of its own (lamehip_batch_set_stream_in_samplerate): "
             "such a batch is fed with appends, the one-shot converter is single-rate", who);
    return -1;
}

/* row ch of stream s in the input pool / in its pinned mirror */
static unsigned char *
batch_pool_row(const lamehip_batch * b, int s, int ch)
{
    return (unsigned char *) b->d_pcm.get() + ((size_t) s * 2 + (size_t) ch) * (size_t) b->cap * (size_t) b->esz;
}

static unsigned char *
batch_mirror_row(const lamehip_batch * b, int s, int ch)
{
    return (unsigned char *) b->h_pcm.get() + ((size_t) s * 2 + (size_t) ch) * (size_t) b->cap * (size_t) b->esz;
}

/* bytes of the whole input pool */
static size_t
batch_pool_bytes(const lamehip_batch * b)
{
    return (size_t) b->B * 2 * (size_t) b->cap * (size_t) b->esz;
}

/* statistics: stream s's table in HBM, or all of them (s < 0), zeroed on the batch's stream; the host copy is stale then */
static int
batch_stats_zero(lamehip_batch * b, int s)
{
    if (!b->st_on)
        return 0;
    if (s < 0)
        HIPCHK(hipMemsetAsync(b->d_st_carry.get(), 0, (size_t) b->B * sizeof(LhStatCarry), b->stream));
    else
        HIPCHK(hipMemsetAsync(b->d_st_carry.get() + s, 0, sizeof(LhStatCarry), b->stream));
    b->st_have = 0;
    return 0;
}

/* every stream back to its initial state: a device-to-device copy of the pristine image on the batch's own
 * stream (a host copy on the null stream would wait for every other batch's work in flight) */
static int
batch_reset_states(lamehip_batch * b)
{
    if (!b->d_state0.get()) {
        std::vector < LhStreamState > s((size_t) b->B);
        for (int i = 0; i < b->B; i++)
            lh_state_init(&s[(size_t) i], &b->cfg);
        HIPCHK(b->d_state0.alloc(s.size()));
        HIPCHK(hipMemcpy(b->d_state0.get(), s.data(), s.size() * sizeof(LhStreamState), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpyAsync(b->d_state.get(), b->d_state0.get(), (size_t) b->B * sizeof(LhStreamState), hipMemcpyDeviceToDevice, b->stream));
    b->encoded = 0;
    return 0;
}

extern "C" lamehip_batch *
lamehip_batch_create(const lame_t proto, int nstreams, long capacity_samples)
{
    int     dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        dev = 0;
    return lamehip_batch_create_on(dev, proto, nstreams, capacity_samples);
}

/* a batch on HIP device `device' (its pools, state, stream and launches live there whatever device
 * is current in the calling thread); the handle only provides the settings and may belong to
 * another device */
extern "C" lamehip_batch *
lamehip_batch_create_on(int device, const lame_t proto, int nstreams, long capacity_samples)
{
    lamehip_batch *b;
    if (device < 0 || device >= lamehip_device_count()) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_create_on: no HIP device %d", device);
        return nullptr;
    }
    LhDeviceScope const on_device(device);
    if (!valid(proto) || !proto->inited || !proto->have_device || nstreams <= 0
        || capacity_samples <= 0) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_create: need an initialised handle on a HIP device");
        return nullptr;
    }
    b = new(std::nothrow) lamehip_batch();
    if (!b)
        return nullptr;
    b->device = device;
    b->cfg = proto->cfg;
    b->user_p = proto->p;
    b->tab = (LhTables *) malloc(sizeof(LhTables));
    if (!b->tab) {
        delete  b;
        return nullptr;
    }
    memcpy(b->tab, proto->tab, sizeof(LhTables));
    b->B = nstreams;
    b->cap = capacity_samples;
    b->len.assign((size_t) nstreams, 0);
    b->nframes.assign((size_t) nstreams, 0);
    b->out_off.assign((size_t) nstreams, 0);
    b->h_desc.resize((size_t) nstreams);
    b->bytes_off.assign((size_t) nstreams, 0);
    b->padding.assign((size_t) nstreams, 0);
    b->row_dirty.assign((size_t) nstreams, 0);
    b->rg_dirty.assign((size_t) nstreams, 0);
    b->rg_len_in.assign((size_t) nstreams, 0);
    b->split = batch_use_split();
    if (proto->rs) {
        /* the s16 pool shrinks to nothing, the converted signal (plus the flush's tail) lives in a float pool */
        b->rate_in = proto->p.samplerate;
        b->rs = (LhResampler *) malloc(sizeof(LhResampler));
        b->capf = (long) ((double) capacity_samples / proto->rs->ratio) + 4 * 1152 + 64;
        capacity_samples = 1;
        if (!b->rs || b->d_pcmf.alloc((size_t) nstreams * 2 * (size_t) b->capf) != hipSuccess) {
            snprintf(g_err, sizeof(g_err), "lamehip_batch_create: device allocation failed");
            lamehip_batch_destroy(b);
            return nullptr;
        }
    }
    if (b->dc.upload(b->cfg, *b->tab) != 0
        || b->d_pcm.alloc((size_t) nstreams * 2 * (size_t) capacity_samples) != hipSuccess
        || b->d_state.alloc((size_t) nstreams) != hipSuccess
        || b->d_desc.alloc((size_t) nstreams) != hipSuccess
        || b->stream.create() != hipSuccess
        || b->ev0.create() != hipSuccess || b->ev1.create() != hipSuccess
        || hipMemset(b->d_pcm.get(), 0, (size_t) nstreams * 2 * (size_t) capacity_samples * 2) != hipSuccess
        || batch_reset_states(b) != 0) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_create: device allocation failed");
        lamehip_batch_destroy(b);
        return nullptr;
    }
    return b;
}

extern "C" void
lamehip_batch_destroy(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return;
    for (size_t i = 0; i < b->packer.size(); i++)
        lh_bs_free(&b->packer[i]);
    lh_rs_trunk_free(&b->trunk);
    for (int c = 1; c < b->rs_ncls; c++)
        free(b->rs_cls[c]);
    free(b->rs);
    free(b->tab);
    b->dc.release();
    delete  b;                  /* (what the owners hold goes here, on the batch's device) */
}

/* Device conversion: stream s will be n input samples long.  The host plans -- the trunk grows to the stream's full
 * chunks, the stream's own last blocks are kept with it -- and with that knows the converted length, the frame count
 * and the end padding; the samples are not looked at. */
static int
batch_plan_stream(lamehip_batch * b, int s, long n)
{
    int const fs = fs_of(b->cfg);
    std::vector < LhRsBlock > &tail = b->tail[(size_t) s];
    long    conv = 0;
    int     frames = 0, padding = 0, ntail;
    if (lh_rs_trunk_extend(b->rs, &b->trunk, n / fs) != 0) {
        snprintf(g_err, sizeof(g_err), "out of memory (conversion plan)");
        return -2;
    }
    tail.resize(16);
    ntail = lh_rs_plan_tail(b->rs, &b->trunk, n, tail.data(), (int) tail.size(), &conv, &frames, &padding);
    if (ntail > (int) tail.size()) {
        tail.resize((size_t) ntail);
        ntail = lh_rs_plan_tail(b->rs, &b->trunk, n, tail.data(), (int) tail.size(), &conv, &frames, &padding);
    }
    if (ntail < 0)
        return -1;
    tail.resize((size_t) ntail);
    if (conv > b->capf) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_pcm: converted stream (%ld samples) exceeds the pool", conv);
        return -1;
    }
    /* (the kernel stages a block's span of input in LDS: nothing the converter cuts is longer than LH_RS_SPAN_MAX, a
     * block being at most 1152 input samples and the taps before them; checked all the same, before anything runs) */
    for (const LhRsBlock & k:tail) {
        if (k.made > 0 && lh_rs_locate(b->rs->ratio, b->rs->taps, b->rs->phases, k.start, k.made - 1).first + b->rs->taps + 1
            - lh_rs_locate(b->rs->ratio, b->rs->taps, b->rs->phases, k.start, 0).first > LH_RS_SPAN_MAX) {
            snprintf(g_err, sizeof(g_err), "conversion plan: a block spans more input than the device kernel stages");
            return -1;
        }
    }
    b->len_in[(size_t) s] = n;
    b->len[(size_t) s] = conv;
    b->nframes[(size_t) s] = frames;
    b->padding[(size_t) s] = padding;
    b->rs_dirty[(size_t) s] = 1;
    return 0;
}

/* input samples of stream s in the s16 pool */
static long
batch_len_in(const lamehip_batch * b, int s)
{
    return b->dev_rs ? b->len_in[(size_t) s] : b->len[(size_t) s];
}

extern "C" int
lamehip_batch_set_length(lamehip_batch * b, int s, long n)
{
    if (!b || s < 0 || s >= b->B || n < 0 || (b->rate_in && !b->dev_rs))
        return -1;              /* (a batch that converts on the host needs the samples themselves: lamehip_batch_set_pcm) */
    if (batch_refuse_own_rates(b, "lamehip_batch_set_length"))
        return -1;
    if (n > b->cap) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_length: stream of %ld samples exceeds the pool (%ld per stream)", n, b->cap);
        return -1;
    }
    b->pcm_given = 1;
    b->rg_dirty[(size_t) s] = 1;        /* declared: the stream's gain is measured again */
    if (b->dev_rs)
        return batch_plan_stream(b, s, n);
    if (b->stype != LH_PCM_S16)
        b->in_dirty[(size_t) s] = 1;    /* declared: the stream is ingested again */
    b->len[(size_t) s] = n;
    b->nframes[(size_t) s] = lh_total_frames_fs(n, fs_of(b->cfg));
    return 0;
}

/* A stream of a converting batch: what the reference makes of it when its frontend feeds
 * lame_encode_buffer 1152 input samples at a time and then flushes (lame.c:1708-1772, 2075-2120;
 * the same bookkeeping as the handle path above, without a device in the loop). */
static int
batch_convert_stream(lamehip_batch * b, int s, const short *l, const short *r, long n)
{
    float  *ol = nullptr, *orr = nullptr;
    long    conv = 0;
    int     frames = 0, padding = 0;
    if (lh_rs_convert_stream(b->rs, b->rate_in, b->cfg.samplerate, fs_of(b->cfg), mfn_of(b->cfg), b->cfg.channels, b->cfg.pcm_scale,
                             b->cfg.pcm_mix, b->cfg.pcm_scale_r, l, r, n, &ol, &orr, &conv, &frames, &padding) != 0) {
        snprintf(g_err, sizeof(g_err), "out of memory (sample rate converter)");
        return -2;
    }
    if (conv > b->capf) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_pcm: converted stream (%ld samples) exceeds the pool", conv);
        lh_rs_free(ol);
        lh_rs_free(orr);
        return -1;
    }
    b->len[(size_t) s] = conv;
    b->nframes[(size_t) s] = frames;
    b->padding[(size_t) s] = padding;
    b->rg_len_in[(size_t) s] = n;
    b->rg_dirty[(size_t) s] = 1;
    hipError_t e = hipSuccess;
    if (conv > 0) {
        e = hipMemcpy(b->d_pcmf.get() + ((size_t) s * 2) * (size_t) b->capf, ol, (size_t) conv * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(b->d_pcmf.get() + ((size_t) s * 2 + 1) * (size_t) b->capf, orr, (size_t) conv * sizeof(float), hipMemcpyHostToDevice);
    }
    lh_rs_free(ol);
    lh_rs_free(orr);
    if (e != hipSuccess)
        return set_err("hipMemcpy", e);
    return 0;
}


/* the mirror for lamehip_batch_set_pcm: made on first use unless the pool is larger than LAMEHIP_PINNED_MAX_MB
 * (default 4096) of pinned host memory */
static int16_t *
batch_host_pool(lamehip_batch * b)
{
    if (!b->h_pcm.get() && (!b->rate_in || b->dev_rs)) {
        const char *e = getenv("LAMEHIP_PINNED_MAX_MB");
        double const limit = (e ? atof(e) : 4096.0) * 1048576.0;
        if ((double) batch_pool_bytes(b) > limit)
            return nullptr;
        (void) lamehip_batch_input_host_ptr(b);
    }
    return b->h_pcm.get();
}

/* the pinned mirror is about to be rewritten by the host: an upload out of it that is still on its way must have
 * finished (the device-side wait in lamehip_batch_encode says nothing to the host) */
static int
batch_mirror_quiesce(lamehip_batch * b)
{
    if (b->up_inflight) {
        HIPCHK(hipEventSynchronize(b->ev_up));
        b->up_inflight = 0;
    }
    return 0;
}

extern "C" int
lamehip_batch_set_pcm(lamehip_batch * b, int s, const short *l, const short *r, long n)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (batch_refuse_own_rates(b, "lamehip_batch_set_pcm"))
        return -1;
    if (b && b->stype != LH_PCM_S16) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_pcm: this batch's sample type is not s16 (lamehip_batch_set_input takes its samples)");
        return -1;
    }
    if (b && b->rate_in && !b->dev_rs) {
        if (s < 0 || s >= b->B || n < 0)
            return -1;
        b->pcm_given = 1;
        if (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f)
            r = l;
        return batch_convert_stream(b, s, l, r, n);
    }
    if (lamehip_batch_set_length(b, s, n) != 0)
        return -1;
    if (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f)
        r = l;                  /* mono: the second plane mirrors the first, the kernel never uses it */
    if (batch_host_pool(b) != nullptr) {
        if (batch_mirror_quiesce(b) != 0)
            return LAMEHIP_ERR_DEVICE;
        /* into the pinned mirror; the rows travel with the next lamehip_batch_upload / _encode, all streams'
         * in one asynchronous copy (the reference's seam: lame_encode_buffer copies into mfbuf, lame.c:1672) */
        memcpy(b->h_pcm.get() + ((size_t) s * 2) * (size_t) b->cap, l, (size_t) n * 2);
        memcpy(b->h_pcm.get() + ((size_t) s * 2 + 1) * (size_t) b->cap, r, (size_t) n * 2);
        if (!b->row_dirty[(size_t) s]) {
            b->row_dirty[(size_t) s] = 1;
            b->n_dirty++;
        }
        return 0;
    }
    /* the pool is too large to mirror in pinned memory: straight to HBM, stream by stream */
    HIPCHK(hipMemcpy(b->d_pcm.get() + ((size_t) s * 2) * (size_t) b->cap, l, (size_t) n * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->d_pcm.get() + ((size_t) s * 2 + 1) * (size_t) b->cap, r, (size_t) n * 2, hipMemcpyHostToDevice));
    return 0;
}

/* The pinned mirror of the batch's s16 pool, [stream][2][capacity] like the pool itself: the caller may
 * decode straight into it (then lamehip_batch_set_length + lamehip_batch_mark_pcm, or lamehip_batch_set_pcm,
 * which copies into it).  NULL for a converting batch or when the mirror cannot be had. */
extern "C" void *
lamehip_batch_input_host_ptr(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return nullptr;
    if (!b->h_pcm.get() && (!b->rate_in || b->dev_rs) && b->h_pcm.alloc(batch_pool_bytes(b) / sizeof(int16_t)) != hipSuccess)
        (void) hipGetLastError();
    /* whoever asks for the pointer is about to write through it: no upload may still be reading the mirror.  (A caller
     * that keeps the pointer across rounds asks again -- or calls lamehip_batch_set_pcm -- before it rewrites rows that
     * an asynchronous lamehip_batch_upload / _encode has taken.) */
    if (b->h_pcm.get() && batch_mirror_quiesce(b) != 0)
        return nullptr;
    if (b->h_pcm.get())
        b->pcm_given = 1;
    return b->h_pcm.get();
}

/* the mirror of an s16 batch as shorts; NULL for any other sample type (lamehip_batch_input_host_ptr) */
extern "C" short *
lamehip_batch_pcm_host_ptr(lamehip_batch * b)
{
    if (b && b->stype != LH_PCM_S16) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_pcm_host_ptr: this batch's sample type is not s16 (lamehip_batch_input_host_ptr)");
        return nullptr;
    }
    return (short *) lamehip_batch_input_host_ptr(b);
}

/* stream s's rows of the mirror were written by the caller: they travel with the next upload */
extern "C" int
lamehip_batch_mark_pcm(lamehip_batch * b, int s)
{
    if (!b || s < 0 || s >= b->B || !b->h_pcm.get())
        return -1;
    b->rg_dirty[(size_t) s] = 1;        /* new samples: the stream's gain is measured again */
    if (b->dev_rs)
        b->rs_dirty[(size_t) s] = 1;    /* new samples: the stream is converted again */
    else if (b->stype != LH_PCM_S16)
        b->in_dirty[(size_t) s] = 1;    /* ... or ingested again */
    if (!b->row_dirty[(size_t) s]) {
        b->row_dirty[(size_t) s] = 1;
        b->n_dirty++;
    }
    return 0;
}

/* Asynchronous H2D of everything that changed in the mirror, on the batch's stream (lamehip_batch_encode does
 * this itself when something is pending).  One copy when every stream changed and the streams fill their rows,
 * else one per row. */
static int
batch_copy_streams(lamehip_batch * b)
{
    if (!b->up_stream) {
        HIPCHK(b->up_stream.create(hipStreamNonBlocking));
        HIPCHK(b->down_stream.create(hipStreamNonBlocking));
        HIPCHK(b->ev_up.create(hipEventDisableTiming));
        HIPCHK(b->ev_sum.create(hipEventDisableTiming));
        HIPCHK(b->ev_down.create(hipEventDisableTiming));
    }
    return 0;
}

extern "C" int
lamehip_batch_upload(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->n_dirty == 0 || !b->h_pcm.get())
        return 0;
    if (batch_copy_streams(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    /* the pool may still be read by the kernel of the previous round (also after a reset, which clears `encoded') */
    if (b->launched)
        HIPCHK(hipStreamWaitEvent(b->up_stream, b->ev1, 0));
    {
        long long used = 0;
        for (int s = 0; s < b->B; s++)
            used += batch_len_in(b, s);
        if (b->n_dirty == b->B && used * 10 >= (long long) b->B * b->cap * 9)
            HIPCHK(hipMemcpyAsync(b->d_pcm.get(), b->h_pcm.get(), batch_pool_bytes(b), hipMemcpyHostToDevice, b->up_stream));
        else
            for (int s = 0; s < b->B; s++) {
                size_t const n = (size_t) batch_len_in(b, s) * (size_t) b->esz;
                if (!b->row_dirty[(size_t) s] || n == 0)
                    continue;
                for (int ch = 0; ch < 2; ch++)
                    HIPCHK(hipMemcpyAsync(batch_pool_row(b, s, ch), batch_mirror_row(b, s, ch), n, hipMemcpyHostToDevice, b->up_stream));
            }
    }
    HIPCHK(hipEventRecord(b->ev_up, b->up_stream));
    b->up_pending = 1;
    b->up_inflight = 1;
    b->row_dirty.assign((size_t) b->B, 0);
    b->n_dirty = 0;
    return 0;
}

/* Samples of the batch's own type from host buffers: l and r advance by `stride' elements per sample (1: planar; 2:
 * interleaved, r = l + 1, as lame_encode_buffer_interleaved* is called).  What lamehip_batch_set_pcm does for shorts. */
extern "C" int
lamehip_batch_set_input(lamehip_batch * b, int s, const void *l, const void *r, int stride, long n)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b || s < 0 || s >= b->B || n < 0 || (stride != 1 && stride != 2)) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_input: no such stream, a negative length or a stride other than 1 or 2");
        return -1;
    }
    if (batch_refuse_own_rates(b, "lamehip_batch_set_input"))
        return -1;
    bool const one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    if (one_plane)
        r = l;                  /* mono: the second plane mirrors the first, the kernel never uses it */
    if (n > 0 && (!l || !r))
        return -1;
    if (b->rate_in && !b->dev_rs) {
        /* (a batch that converts on the host is s16: lamehip_batch_set_sample_type) */
        std::vector < short >tl((size_t) n + 1), tr((size_t) n + 1);
        lh_pcm_copy_plane(tl.data(), l, 2, stride, n);
        lh_pcm_copy_plane(tr.data(), r, 2, stride, n);
        return lamehip_batch_set_pcm(b, s, tl.data(), tr.data(), n);
    }
    if (lamehip_batch_set_length(b, s, n) != 0)
        return -1;
    if (batch_host_pool(b) != nullptr) {
        if (batch_mirror_quiesce(b) != 0)
            return LAMEHIP_ERR_DEVICE;
        lh_pcm_copy_plane(batch_mirror_row(b, s, 0), l, b->esz, stride, n);
        lh_pcm_copy_plane(batch_mirror_row(b, s, 1), r, b->esz, stride, n);
        if (!b->row_dirty[(size_t) s]) {
            b->row_dirty[(size_t) s] = 1;
            b->n_dirty++;
        }
        return 0;
    }
    /* the pool is too large to mirror in pinned memory: straight to HBM, stream by stream */
    std::vector < unsigned char >tmp;
    for (int ch = 0; ch < 2; ch++) {
        const void *src = ch ? r : l;
        if (stride != 1) {
            tmp.resize((size_t) n * (size_t) b->esz + 1);
            lh_pcm_copy_plane(tmp.data(), src, b->esz, stride, n);
            src = tmp.data();
        }
        if (n > 0)
            HIPCHK(hipMemcpy(batch_pool_row(b, s, ch), src, (size_t) n * (size_t) b->esz, hipMemcpyHostToDevice));
    }
    return 0;
}

/* the same from buffers in HBM, synchronous: stride 1 is two device-to-device copies, stride 2 a kernel that takes the
 * interleaved buffer apart (lh_ingest.hip) */
extern "C" int
lamehip_batch_set_input_device(lamehip_batch * b, int s, const void *dl, const void *dr, int stride, long n)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (b && stride != 1 && stride != 2) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_input_device: stride %d (1: planar, 2: interleaved)", stride);
        return -1;
    }
    if (batch_refuse_own_rates(b, "lamehip_batch_set_input_device"))
        return -1;
    if (lamehip_batch_set_length(b, s, n) != 0)
        return -1;
    bool const one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    if (one_plane)
        dr = dl;
    if (n > 0 && (!dl || !dr))
        return -1;
    if (b->up_pending || b->up_inflight) {      /* an upload of the mirror is on its way into the same pool */
        HIPCHK(hipStreamSynchronize(b->up_stream));
        b->up_inflight = 0;
    }
    if (b->row_dirty[(size_t) s]) {     /* what the mirror holds for this stream is superseded */
        b->row_dirty[(size_t) s] = 0;
        b->n_dirty--;
    }
    if (n == 0)
        return 0;
    if (stride == 1) {
        HIPCHK(hipMemcpy(batch_pool_row(b, s, 0), dl, (size_t) n * (size_t) b->esz, hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(batch_pool_row(b, s, 1), dr, (size_t) n * (size_t) b->esz, hipMemcpyDeviceToDevice));
        return 0;
    }
    /* (on the batch's stream: behind a kernel of the previous round that may still be reading the pool) */
    int const rc = lh_launch_deinterleave(b->esz, dl, dr, batch_pool_row(b, s, 0), one_plane ? nullptr : batch_pool_row(b, s, 1),
                                          n, (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("de-interleave launch", (hipError_t) rc);
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

extern "C" int
lamehip_batch_set_pcm_device(lamehip_batch * b, int s, const void *dl, const void *dr, long n)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (b && b->stype != LH_PCM_S16) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_pcm_device: this batch's sample type is not s16 (lamehip_batch_set_input_device)");
        return -1;
    }
    if (batch_refuse_own_rates(b, "lamehip_batch_set_pcm_device"))
        return -1;
    if (lamehip_batch_set_length(b, s, n) != 0)
        return -1;
    if (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f)
        dr = dl;
    if (b->up_pending || b->up_inflight) {      /* an upload of the mirror is on its way into the same pool */
        HIPCHK(hipStreamSynchronize(b->up_stream));
        b->up_inflight = 0;
    }
    if (b->row_dirty[(size_t) s]) {     /* what the mirror holds for this stream is superseded */
        b->row_dirty[(size_t) s] = 0;
        b->n_dirty--;
    }
    HIPCHK(hipMemcpy(b->d_pcm.get() + ((size_t) s * 2) * (size_t) b->cap, dl, (size_t) n * 2, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(b->d_pcm.get() + ((size_t) s * 2 + 1) * (size_t) b->cap, dr, (size_t) n * 2, hipMemcpyDeviceToDevice));
    return 0;
}

extern "C" void *
lamehip_batch_pcm_device_ptr(lamehip_batch * b)
{
    return (b && (!b->rate_in || b->dev_rs)) ? (void *) b->d_pcm.get() : nullptr;
}


/* ---- incremental use of a batch: lame_encode_buffer semantics for many streams at once -------
 * (reference lame.c:1672-1775: every call appends samples to a stream and encodes the frames that
 * became complete; the output lags the input by the priming).  lamehip_batch_append stages a chunk
 * per stream in pinned host memory, lamehip_batch_encode_available moves all staged chunks to HBM
 * with ONE asynchronous copy, encodes every stream's newly complete frames with ONE launch and packs
 * them, lamehip_batch_drain hands a stream's new bytes over -- the bytes lame_encode_buffer would
 * have returned for the same calls --, lamehip_batch_finish is lame_encode_flush for all streams. */
static int
batch_incremental_check(const lamehip_batch * b, const char *who, int typed_ok)
{
    if (b->incremental)
        return 0;
    /* (typed_ok: entered through lamehip_batch_append_input / _append_input_device / _append_device, which take the batch's
     * own element type) */
    if (b->stype != LH_PCM_S16 && !typed_ok) {
        snprintf(g_err, sizeof(g_err), "%s: lamehip_batch_append and what follows it start an s16 batch, this batch's sample type is not s16 "
                 "(lamehip_batch_append_input takes its samples)", who);
        return -1;
    }
    /* (how the reference converts the rate depends on how it is called, chunk by chunk: the conversion plan of a batch is
     * made for whole streams, unless lamehip_batch_set_incremental_resampling asked for the plan that follows the calls) */
    if ((b->rate_in && !b->inc_rs) || (b->dev_pack && !b->inc_pack)) {
        snprintf(g_err, sizeof(g_err), "%s: incremental batches take the encoder's own input rate and the host packer, this batch %s", who,
                 !b->rate_in || b->inc_rs ? "packs on the device (lamehip_batch_set_device_packing)"
                 : b->dev_rs ? "converts the sample rate (lamehip_batch_set_incremental_resampling lets it do so round by round)"
                 : "converts the sample rate");
        return -1;
    }
    return 0;
}

/* A batch that measures ReplayGain round by round starts (over): every stream's analysis in front of its first sample --
 * cursors, the blocks planned, the carry in HBM (on the batch's stream, in front of the first round's launch) --, no window,
 * no gain; whatever lamehip_batch_encode measured of whole streams before the first append is forgotten. */
static int
batch_gain_restart(lamehip_batch * b)
{
    if (!b->inc_rg)
        return 0;
    HIPCHK(hipMemsetAsync(b->d_rg_carry.get(), 0, (size_t) b->B * sizeof(LhGainCarry), b->stream));
    for (LhGainCursor & c:b->rg_cur)
        lh_gain_cursor_init(&c);
    for (std::vector < int >&g:b->rg_blk)
        g.clear();
    b->rg_heard.assign((size_t) b->B, 0);
    for (std::vector < double >&w:b->rg_win)
        w.clear();
    b->rg_tenths.assign((size_t) b->B, 0);
    b->rg_final.assign((size_t) b->B, 0);
    b->rg_closed = 0;
    b->rg_measured = 0;
    b->rg_pending = 0;
    b->rg_ran = 0;
    b->rg_ms = 0;
    return 0;
}

static int batch_frame_max(const lamehip_batch * b);

/* An incremental batch that packs on the device starts (over): the byte pool laid out -- once: every stream's slice holds
 * the frames of a stream as long as the batch's capacity (the converted capacity when the batch converts), each as large as
 * the settings allow, and never moves --, nothing handed out, every stream's header walk (lh_drain.hip) at its first byte. */
static int
batch_drain_begin(lamehip_batch * b)
{
    int const frame_max = batch_frame_max(b);
    long long const slice = (long long) lh_total_frames_fs(b->inc_rs ? b->capf : b->cap, fs_of(b->cfg)) * frame_max;
    HIPCHK(b->d_bytes.reserve((size_t) b->B * (size_t) slice));
    HIPCHK(hipMemsetAsync(b->d_dr_carry.get(), 0, (size_t) b->B * sizeof(long long), b->stream));
    if (b->inc_tag) {
        /* (with tag frames: every stream's carry in front of its first byte and frame, no frame to hand out) */
        HIPCHK(hipMemsetAsync(b->d_tg_carry.get(), 0, (size_t) b->B * sizeof(LhTagCarry), b->stream));
        b->tg_patched.assign((size_t) b->B, 0);
        b->tg_has.assign((size_t) b->B, 0);
        b->tg_have = 0;
        b->tg_ran = 0;
        b->tag_ms = 0;
    }
    b->dr_slice = slice;
    b->dr_frame_max = frame_max;
    b->dr_drained.assign((size_t) b->B, 0);
    b->dr_next.assign((size_t) b->B, 0);
    b->dr_done.assign((size_t) b->B, 0);
    for (int s = 0; s < b->B; s++)
        b->bytes_off[(size_t) s] = (long long) s * slice;
    b->dr_have = 0;
    b->dr_ran = 0;
    b->dr_ms = 0;
    return 0;
}

/* every slot holds a live stream in front of its first sample, and no restart is owed (the records in HBM are put back whole
 * by whoever calls this) */
static void
batch_slots_open(lamehip_batch * b)
{
    b->slot.assign((size_t) b->B, (char) LH_SLOT_LIVE);
    b->ending.assign((size_t) b->B, 0);
    b->sl_list.clear();
    b->sl_ran = 0;
    b->sl_gap = 0;
    b->sl_ms = 0;
}

/* stream s takes samples: it has not been ended (lamehip_batch_end_stream), or its slot has been restarted since */
static int
batch_slot_takes(const lamehip_batch * b, const char *who, int s)
{
    if (b->slot.empty() || b->slot[(size_t) s] == LH_SLOT_LIVE)
        return 1;
    snprintf(g_err, sizeof(g_err), "%s: stream %d %s (lamehip_batch_end_stream): lamehip_batch_restart_stream gives its slot to the next "
             "stream", who, s, b->slot[(size_t) s] == LH_SLOT_ENDING ? "ends with the next round" : "has ended");
    return 0;
}

static int
batch_incremental_begin(lamehip_batch * b, const char *who, int typed_ok)
{
    if (b->incremental)
        return 0;
    if (batch_incremental_check(b, who, typed_ok) != 0)
        return -1;
    if (b->inc_pack && batch_drain_begin(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    if (batch_reset_states(b) != 0 || batch_gain_restart(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    batch_slots_open(b);
    b->handed.assign((size_t) b->B, std::vector < unsigned char >());
    b->fed.assign((size_t) b->B, 0);
    b->done.assign((size_t) b->B, 0);
    b->staged.assign((size_t) b->B, 0);
    b->pending.assign((size_t) b->B, std::vector < unsigned char >());
    b->last.resize((size_t) b->B);
    b->have_last.assign((size_t) b->B, 0);
    b->packer.resize((size_t) b->B);
    for (int s = 0; s < b->B; s++)
        if (lh_bs_init_sized(&b->packer[(size_t) s], 65536) != 0)
            return -2;
    b->incremental = 1;
    return 0;
}

/* a batch that measures ReplayGain is encoded whole (lamehip_batch_encode): the analysis runs once per stream -- refused
 * unless lamehip_batch_set_incremental_replaygain has the analysis follow the calls */
static int
batch_refuse_gain(const lamehip_batch * b, const char *who)
{
    if (!b->rg_on || b->inc_rg) /* (lamehip_batch_set_incremental_replaygain: measured round by round) */
        return 0;
    snprintf(g_err, sizeof(g_err), "%s: this batch measures ReplayGain (lamehip_batch_set_replaygain), which incremental use does not", who);
    return 1;
}

#define LH_STAGE_SEGS 4096       /* chunks per trip to HBM */
#define LH_STAGE_SAMPLES (8L << 20)     /* the arena: 8 M samples = 16 MB; what is staged beyond goes to HBM at once */

/* the staging area, made once: descriptors, chunk table, arena */
static int
batch_stage_reserve(lamehip_batch * b)
{
    long const arena_at = ((long) b->B * (long) sizeof(LhStreamDesc) + (long) LH_STAGE_SEGS * 16 + 63) & ~63L;
    long const bytes = arena_at + LH_STAGE_SAMPLES * 2;
    if (b->h_stage.get())
        return 0;
    if (b->h_stage.alloc((size_t) bytes) != hipSuccess || b->d_stage.alloc((size_t) bytes) != hipSuccess) {
        b->h_stage.release();   /* (both or neither) */
        return set_err("staging allocation", hipErrorOutOfMemory);
    }
    b->stage_arena_at = arena_at;
    b->stage_cap = LH_STAGE_SAMPLES;
    b->stage_used = 0;
    b->stage_nseg = 0;
    return 0;
}

/* the segment table of the typed / device-resident appends and the events around their launches, made once */
static int
batch_append_reserve(lamehip_batch * b)
{
    size_t const n = (size_t) LH_STAGE_SEGS + (size_t) b->B;
    LhPinned < LhApSeg > h;
    LhDevBuf < LhApSeg > d;
    LhEvent ev[2];
    if (b->h_ap.get())
        return 0;
    /* everything new first: a failure leaves the batch as it was */
    hipError_t e = h.alloc(n);
    if (e == hipSuccess)
        e = d.alloc(n);
    if (e == hipSuccess)
        e = ev[0].create();
    if (e == hipSuccess)
        e = ev[1].create();
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("append table allocation", e);
    }
    b->h_ap = std::move(h);
    b->d_ap = std::move(d);
    b->ev_ap[0] = std::move(ev[0]);
    b->ev_ap[1] = std::move(ev[1]);
    return 0;
}

/* the time of the append launch ev_ap[] are around joins ap_ms (the launch has finished, or is waited for here) */
static void
batch_append_time(lamehip_batch * b)
{
    float   ms = 0;
    if (!b->ap_timed)
        return;
    b->ap_timed = 0;
    if (hipEventSynchronize(b->ev_ap[1]) == hipSuccess && hipEventElapsedTime(&ms, b->ev_ap[0], b->ev_ap[1]) == hipSuccess)
        b->ap_ms += ms;
    else
        (void) hipGetLastError();
}

/* nsegs entries of the table at `segs' (HBM), the longest of max_n samples, go to the pool the kernels read -- the float
 * pool of a typed batch, through lame_copy_inbuffer's arithmetic, or the s16 pool as they are --: one launch of
 * lh_append_kernel on the batch's stream, between ev_ap[0] and ev_ap[1] */
static int
batch_append_launch(lamehip_batch * b, const LhApSeg * segs, int nsegs, long long max_n)
{
    LhInParams p;
    if (nsegs <= 0 || max_n <= 0)
        return 0;
    batch_append_time(b);       /* (the events are about to be recorded again) */
    memset(&p, 0, sizeof(p));
    p.m = lh_pcm_matrix(b->stype, b->cfg.pcm_scale, b->cfg.pcm_mix, b->cfg.pcm_scale_r);
    p.channels = b->cfg.channels;
    p.one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    p.cap = b->cap;
    HIPCHK(hipEventRecord(b->ev_ap[0], b->stream));
    /* (a batch that converts round by round: into the input pool as they are, the converter reads them there) */
    int const rc = b->inc_rs ? lh_launch_append_raw(b->esz, &p, segs, nsegs, max_n, (void *) b->d_pcm.get(), (void *) (hipStream_t) b->stream)
        : lh_launch_append(b->stype, &p, segs, nsegs, max_n,
                           b->stype == LH_PCM_S16 ? (void *) b->d_pcm.get() : (void *) b->d_pcmf.get(), (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("append launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_ap[1], b->stream));
    b->ap_timed = 1;
    return 0;
}

/* what is staged goes to the pool: one copy of the chunk table and of the arena's bytes in use, one scatter
 * launch; wait = the arena is free again on return (it is about to be refilled) */
static int
batch_stage_flush(lamehip_batch * b, int wait)
{
    size_t const segs_at = (size_t) b->B * sizeof(LhStreamDesc);
    if (b->stage_nseg > 0 || b->ap_nseg > 0) {
        int     rc;
        if (b->stage_nseg > 0)
            HIPCHK(hipMemcpyAsync(b->d_stage.get() + segs_at, b->h_stage.get() + segs_at, (size_t) b->stage_nseg * 16, hipMemcpyHostToDevice,
                                  b->stream));
        if (b->ap_nseg > 0)
            HIPCHK(hipMemcpyAsync(b->d_ap.get(), b->h_ap.get(), (size_t) b->ap_nseg * sizeof(LhApSeg), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(b->d_stage.get() + b->stage_arena_at, b->h_stage.get() + b->stage_arena_at, (size_t) b->stage_used * 2,
                              hipMemcpyHostToDevice, b->stream));
        rc = lh_launch_scatter((const int16_t *) (b->d_stage.get() + b->stage_arena_at), b->d_pcm.get(), b->cap,
                               (const int *) (b->d_stage.get() + segs_at), b->stage_nseg, (void *) (hipStream_t) b->stream);
        if (rc)
            return set_err("scatter launch", (hipError_t) rc);
        /* (the chunks of lamehip_batch_append_input: other places of the rows than the scatter's) */
        if (b->ap_nseg > 0 && (rc = batch_append_launch(b, b->d_ap.get(), b->ap_nseg, b->ap_max_n)) != 0)
            return rc;
        b->ap_nseg = 0;
        b->ap_max_n = 0;
        for (int s = 0; s < b->B; s++) {
            b->fed[(size_t) s] += b->staged[(size_t) s];
            b->staged[(size_t) s] = 0;
        }
        b->stage_nseg = 0;
        b->stage_used = 0;
        if (wait) {
            HIPCHK(hipStreamSynchronize(b->stream));
            batch_append_time(b);
        }
    }
    return 0;
}

/* A batch that converts round by round: the append of n samples to stream s is one lame_encode_buffer call to the converter,
 * planned here from the stream's cursor.  Refused (-1, `who' in the message) when the stream, flushed right after this call,
 * would not fit its rows of the float pool -- so lamehip_batch_finish never lacks room.  commit: the cursor advances and the
 * call's tiles join the round's list; else the call is only checked, and *ntiles (when given) grows by its tiles.  An
 * allocation failure returns LAMEHIP_ERR_DEVICE; either way a call that does not return 0 leaves the batch as it was. */
static int
batch_rs_plan_append(lamehip_batch * b, const char *who, int s, int n, bool commit, size_t *ntiles = nullptr)
{
    int const fs = fs_of(b->cfg), mfn = mfn_of(b->cfg);
    const LhResampler *const rs = batch_stream_rs(b, s);        /* (the stream's own converter) */
    int const cls = batch_stream_cls(b, s);
    LhRsCursor c = b->rs_cur[(size_t) s], end;
    int     padding = 0;
    size_t  nt = 0;
    int const nblk = lh_rs_plan_call(rs, fs, mfn, &c, n, nullptr, 0);
    try {
        b->rs_blk.resize((size_t) nblk);
    }
    catch(const std::bad_alloc &) {
        snprintf(g_err, sizeof(g_err), "%s: out of memory (conversion plan)", who);
        return LAMEHIP_ERR_DEVICE;
    }
    c = b->rs_cur[(size_t) s];
    (void) lh_rs_plan_call(rs, fs, mfn, &c, n, b->rs_blk.data(), nblk);
    end = c;
    (void) lh_rs_plan_flush(rs, fs, mfn, &end, nullptr, 0, &padding);
    if (end.fed > (long long) b->inc_capf) {
        snprintf(g_err, sizeof(g_err), "%s: stream %d, flushed behind this call, would be %lld converted samples: more than the float pool's "
                 "%ld per stream", who, s, end.fed, b->inc_capf);
        return -1;
    }
    /* (ReplayGain round by round: the analysis hears the converted samples, in the blocks they are made in) */
    if (b->inc_rg) {
        if (end.fed > b->inc_rg_max) {
            snprintf(g_err, sizeof(g_err), "%s: stream %d, flushed behind this call, would be %lld samples: more than the ReplayGain analysis "
                     "takes (%lld)", who, s, end.fed, b->inc_rg_max);
            return -1;
        }
        try {
            b->rg_blk[(size_t) s].reserve(b->rg_blk[(size_t) s].size() + b->rs_blk.size());
        }
        catch(const std::bad_alloc &) {
            snprintf(g_err, sizeof(g_err), "%s: out of memory (gain plan)", who);
            return LAMEHIP_ERR_DEVICE;
        }
    }
    for (const LhRsBlock & k:b->rs_blk)
        nt += (size_t) lh_rs_block_tiles_class(rs, &k, s, cls, nullptr, 0);
    if (ntiles)
        *ntiles += nt;
    if (!commit)
        return 0;
    size_t const at = b->h_tiles.size();
    try {
        b->h_tiles.resize(at + nt);
    }
    catch(const std::bad_alloc &) {
        snprintf(g_err, sizeof(g_err), "%s: out of memory (tile table)", who);
        return LAMEHIP_ERR_DEVICE;
    }
    nt = at;
    for (const LhRsBlock & k:b->rs_blk)
        nt += (size_t) lh_rs_block_tiles_class(rs, &k, s, cls, b->h_tiles.data() + nt, (int) (b->h_tiles.size() - nt));
    if (b->inc_rg)
        for (const LhRsBlock & k:b->rs_blk)
            if (k.made > 0)
                b->rg_blk[(size_t) s].push_back(k.made);        /* (room was made above) */
    b->rs_cur[(size_t) s] = c;
    return 0;
}

/* A batch that measures ReplayGain round by round and does not convert: the append of n samples to stream s is one
 * lame_encode_buffer call to the analysis, planned here from the stream's cursor (lh_gain_plan_call; a batch that converts has
 * it from batch_rs_plan_append).  Refused (-1, `who' in the message) when the stream, flushed right after this call, would be
 * longer than the analysis takes.  commit: the cursor advances and the call's blocks join the round's; else the call is only
 * checked and room made for its blocks.  An allocation failure returns LAMEHIP_ERR_DEVICE; a call that does not return 0
 * leaves the batch as it was. */
static int
batch_rg_plan_append(lamehip_batch * b, const char *who, int s, int n, bool commit)
{
    if (!b->inc_rg || b->inc_rs)
        return 0;
    int const fs = fs_of(b->cfg), mfn = mfn_of(b->cfg);
    LhGainCursor c = b->rg_cur[(size_t) s], end;
    int const nblk = lh_gain_plan_call(&c, fs, mfn, n, nullptr, 0);
    end = c;
    if (nblk < 0 || lh_gain_plan_flush(&end, fs, mfn, nullptr, 0) < 0 || end.heard > b->inc_rg_max) {
        snprintf(g_err, sizeof(g_err), "%s: stream %d, flushed behind this call, would be %lld samples: more than the ReplayGain analysis "
                 "takes (%lld)", who, s, nblk < 0 ? -1LL : end.heard, b->inc_rg_max);
        return -1;
    }
    std::vector < int >&g = b->rg_blk[(size_t) s];
    size_t const at = g.size();
    try {
        g.reserve(at + (size_t) nblk);
    }
    catch(const std::bad_alloc &) {
        snprintf(g_err, sizeof(g_err), "%s: out of memory (gain plan)", who);
        return LAMEHIP_ERR_DEVICE;
    }
    if (!commit)
        return 0;
    g.resize(at + (size_t) nblk);
    (void) lh_gain_plan_call(&b->rg_cur[(size_t) s], fs, mfn, n, g.data() + at, nblk);
    return 0;
}

extern "C" int
lamehip_batch_append(lamehip_batch * b, int s, const short *l, const short *r, int n)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int     rc;
    if (!b || s < 0 || s >= b->B || n < 0 || (n > 0 && !l))
        return -1;
    if (b->finished) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_append: the batch is finished (lamehip_batch_reset starts it over)");
        return -1;
    }
    if (batch_refuse_gain(b, "lamehip_batch_append"))
        return -1;
    if (b->stype != LH_PCM_S16) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_append: takes s16, this batch's sample type is not (lamehip_batch_append_input takes its samples)");
        return -1;
    }
    if ((rc = batch_incremental_begin(b, "lamehip_batch_append", 0)) != 0)
        return rc;
    if (!batch_slot_takes(b, "lamehip_batch_append", s))
        return -1;
    if (n == 0)
        return 0;
    if (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f)
        r = l;
    if (!r)
        return -1;
    if (b->fed[(size_t) s] + b->staged[(size_t) s] + n > b->cap) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_append: stream %d would exceed the batch's capacity of %ld samples", s, b->cap);
        return -1;
    }
    if ((rc = batch_stage_reserve(b)) != 0)
        return rc;
    if ((rc = batch_rg_plan_append(b, "lamehip_batch_append", s, n, false)) != 0)
        return rc;
    if (b->inc_rs && (rc = batch_rs_plan_append(b, "lamehip_batch_append", s, n, true)) != 0)
        return rc;
    (void) batch_rg_plan_append(b, "lamehip_batch_append", s, n, true);
    /* pieces of at most half the arena; when the arena or the chunk table is full, what is staged leaves for HBM */
    while (n > 0) {
        int const piece = ((long) n > b->stage_cap / 4) ? (int) (b->stage_cap / 4) : n;
        int    *seg;
        int16_t *arena = (int16_t *) (b->h_stage.get() + b->stage_arena_at);
        if (b->stage_used + 2L * piece > b->stage_cap || b->stage_nseg == LH_STAGE_SEGS)
            if ((rc = batch_stage_flush(b, 1)) != 0)
                return rc;
        seg = (int *) (b->h_stage.get() + (size_t) b->B * sizeof(LhStreamDesc)) + 4 * b->stage_nseg;
        seg[0] = (int) b->stage_used;
        seg[1] = s;
        seg[2] = (int) (b->fed[(size_t) s] + b->staged[(size_t) s]);
        seg[3] = piece;
        memcpy(arena + b->stage_used, l, (size_t) piece * 2);
        memcpy(arena + b->stage_used + piece, r, (size_t) piece * 2);
        b->stage_used += 2L * piece;
        b->stage_nseg++;
        b->staged[(size_t) s] += piece;
        l += piece;
        r += piece;
        n -= piece;
    }
    return 0;
}

/* ---- appends in the batch's own element type, from host memory or from HBM (any sample type; csrc/lh_ingest.hip:
 * lh_append_kernel).  A chunk's place in its stream's rows is fixed when it is appended, fed + staged: a chunk staged in
 * the arena is counted in `staged' until it leaves for HBM, one that comes from device buffers is in the pool when the call
 * returns and counted in `fed' at once -- so the two kinds may follow each other in any order and land disjointly. ---- */

/* what the three calls check and make ready before they touch anything: 0, or the call's return value */
static int
batch_append_enter(lamehip_batch * b, const char *who, int stride)
{
    int     rc;
    if (b->finished) {
        snprintf(g_err, sizeof(g_err), "%s: the batch is finished (lamehip_batch_reset starts it over)", who);
        return -1;
    }
    if (batch_refuse_gain(b, who))
        return -1;
    if (stride != 1 && stride != 2) {
        snprintf(g_err, sizeof(g_err), "%s: stride %d (1: planar, 2: interleaved)", who, stride);
        return -1;
    }
    if (batch_incremental_check(b, who, 1) != 0)
        return -1;
    if ((rc = batch_stage_reserve(b)) != 0 || (rc = batch_append_reserve(b)) != 0)
        return rc;
    return batch_incremental_begin(b, who, 1);
}

static int
batch_append_fits(const lamehip_batch * b, const char *who, int s, long long n)
{
    if (b->fed[(size_t) s] + b->staged[(size_t) s] + n <= b->cap)
        return 1;
    snprintf(g_err, sizeof(g_err), "%s: stream %d would exceed the batch's capacity of %ld samples", who, s, b->cap);
    return 0;
}

/* Host buffers in the batch's element type, l and r `stride' elements from sample to sample as for lamehip_batch_set_input:
 * staged in the pinned arena like the shorts of lamehip_batch_append -- 16-byte aligned, an interleaved chunk as it is --,
 * on their way to HBM with the next lamehip_batch_encode_available / _finish, or earlier when the arena or the table is full. */
extern "C" int
lamehip_batch_append_input(lamehip_batch * b, int s, const void *l, const void *r, int stride, int n)
{
    static const char who[] = "lamehip_batch_append_input";
    LhDeviceScope const on_device(b ? b->device : -1);
    int     rc;
    if (!b || s < 0 || s >= b->B || n < 0 || (n > 0 && !l)) {
        snprintf(g_err, sizeof(g_err), "%s: no such stream, a negative length or no samples", who);
        return -1;
    }
    if ((rc = batch_append_enter(b, who, stride)) != 0)
        return rc;
    if (!batch_slot_takes(b, who, s))
        return -1;
    if (n == 0)
        return 0;
    bool const one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    if (one_plane)
        r = l;                  /* mono: the second plane mirrors the first, the kernel never reads it */
    if (!r) {
        snprintf(g_err, sizeof(g_err), "%s: no right samples", who);
        return -1;
    }
    if (!batch_append_fits(b, who, s, n))
        return -1;
    if ((rc = batch_rg_plan_append(b, who, s, n, false)) != 0)
        return rc;
    if (b->inc_rs && (rc = batch_rs_plan_append(b, who, s, n, true)) != 0)
        return rc;
    (void) batch_rg_plan_append(b, who, s, n, true);
    long const esz = b->esz;
    bool const inter = (stride == 2 && !one_plane && (const char *) r == (const char *) l + esz);
    /* pieces of at most a quarter of the arena's bytes per plane; when the arena or the table is full, what is staged
     * leaves for HBM */
    while (n > 0) {
        long const piece_max = b->stage_cap / 2 / esz;
        int const piece = (long) n > piece_max ? (int) piece_max : n;
        long const plane = ((long) piece * esz + 15) & ~15L;    /* bytes */
        long const need = (inter ? ((2L * piece * esz + 15) & ~15L) : (one_plane ? plane : 2 * plane)) / 2;     /* shorts */
        long    at = (b->stage_used + 7) & ~7L;
        if (at + need > b->stage_cap || b->ap_nseg == LH_STAGE_SEGS) {
            if ((rc = batch_stage_flush(b, 1)) != 0)
                return rc;
            at = 0;
        }
        unsigned char *const dst = b->h_stage.get() + b->stage_arena_at + at * 2;
        unsigned long long const dev = (unsigned long long) (uintptr_t) (b->d_stage.get() + b->stage_arena_at) + (unsigned long long) at * 2;
        LhApSeg & g = b->h_ap.get()[b->ap_nseg];
        g.at = b->fed[(size_t) s] + b->staged[(size_t) s];
        g.n = piece;
        g.stream = s;
        g.l = dev;
        if (inter) {
            memcpy(dst, l, 2 * (size_t) piece * (size_t) esz);
            g.r = dev + (unsigned long long) esz;
            g.stride = 2;
        }
        else {
            lh_pcm_copy_plane(dst, l, (int) esz, stride, piece);
            if (!one_plane)
                lh_pcm_copy_plane(dst + plane, r, (int) esz, stride, piece);
            g.r = one_plane ? dev : dev + (unsigned long long) plane;
            g.stride = 1;
        }
        b->stage_used = at + need;
        b->ap_nseg++;
        if (piece > b->ap_max_n)
            b->ap_max_n = piece;
        b->staged[(size_t) s] += piece;
        l = (const char *) l + (size_t) piece * (size_t) stride * (size_t) esz;
        r = (const char *) r + (size_t) piece * (size_t) stride * (size_t) esz;
        n -= piece;
    }
    return 0;
}

/* the nsegs entries behind the staged ones in the pinned table (device addresses): one copy of the table, one launch, and
 * the wait for it -- the samples are in the pool and counted on return */
static int
batch_append_resident(lamehip_batch * b, int nsegs, long long max_n)
{
    LhApSeg *const h = b->h_ap.get() + LH_STAGE_SEGS, *const d = b->d_ap.get() + LH_STAGE_SEGS;
    int     rc;
    if (nsegs <= 0)
        return 0;
    HIPCHK(hipMemcpyAsync(d, h, (size_t) nsegs * sizeof(LhApSeg), hipMemcpyHostToDevice, b->stream));
    if ((rc = batch_append_launch(b, d, nsegs, max_n)) != 0)
        return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    batch_append_time(b);
    for (int i = 0; i < nsegs; i++)
        b->fed[(size_t) h[i].stream] += (long) h[i].n;
    return 0;
}

/* the same from buffers in HBM, synchronous like lamehip_batch_set_input_device: whatever produced the buffers must have
 * finished, and the caller may reuse them when the call returns */
extern "C" int
lamehip_batch_append_input_device(lamehip_batch * b, int s, const void *dl, const void *dr, int stride, int n)
{
    static const char who[] = "lamehip_batch_append_input_device";
    LhDeviceScope const on_device(b ? b->device : -1);
    int     rc;
    if (!b || s < 0 || s >= b->B || n < 0 || (n > 0 && !dl)) {
        snprintf(g_err, sizeof(g_err), "%s: no such stream, a negative length or no samples", who);
        return -1;
    }
    if ((rc = batch_append_enter(b, who, stride)) != 0)
        return rc;
    if (!batch_slot_takes(b, who, s))
        return -1;
    if (n == 0)
        return 0;
    if (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f)
        dr = dl;
    if (!dr) {
        snprintf(g_err, sizeof(g_err), "%s: no right samples", who);
        return -1;
    }
    if (!batch_append_fits(b, who, s, n))
        return -1;
    if ((rc = batch_rg_plan_append(b, who, s, n, false)) != 0)
        return rc;
    if (b->inc_rs && (rc = batch_rs_plan_append(b, who, s, n, true)) != 0)
        return rc;
    (void) batch_rg_plan_append(b, who, s, n, true);
    LhApSeg & g = b->h_ap.get()[LH_STAGE_SEGS];
    g.l = (unsigned long long) (uintptr_t) dl;
    g.r = (unsigned long long) (uintptr_t) dr;
    g.at = b->fed[(size_t) s] + b->staged[(size_t) s];
    g.n = n;
    g.stream = s;
    g.stride = stride;
    return batch_append_resident(b, 1, n);
}

/* One round for all streams from one device array (a producer's [B, C, T] tensor): stream s takes nsamples[s] samples, the
 * left ones from element s * stream_stride of `dev' on, the right ones plane_stride elements further on, `stride' elements
 * from sample to sample.  ONE launch for the whole batch; synchronous as above. */
extern "C" int
lamehip_batch_append_device(lamehip_batch * b, const void *dev, long long stream_stride, long long plane_stride, int stride,
                            const int *nsamples)
{
    static const char who[] = "lamehip_batch_append_device";
    LhDeviceScope const on_device(b ? b->device : -1);
    long long max_n = 0;
    int     rc, nsegs = 0;
    if (!b || !nsamples) {
        snprintf(g_err, sizeof(g_err), "%s: no batch or no lengths", who);
        return -1;
    }
    if ((rc = batch_append_enter(b, who, stride)) != 0)
        return rc;
    /* every stream checked before the first is counted: a refused round leaves the batch as it was */
    for (int s = 0; s < b->B; s++) {
        if (nsamples[s] < 0 || (nsamples[s] > 0 && !dev)) {
            snprintf(g_err, sizeof(g_err), "%s: stream %d: a negative length or no samples", who, s);
            return -1;
        }
        /* (a slot whose stream has been ended takes part in the round with no samples) */
        if (nsamples[s] > 0 && !batch_slot_takes(b, who, s))
            return -1;
        if (!batch_append_fits(b, who, s, nsamples[s]))
            return -1;
    }
    /* (the same for the analysis of a batch that measures ReplayGain round by round: checked, room made, then counted) */
    for (int s = 0; s < b->B; s++)
        if (nsamples[s] > 0 && (rc = batch_rg_plan_append(b, who, s, nsamples[s], false)) != 0)
            return rc;
    for (int s = 0; s < b->B && !b->inc_rs; s++)
        if (nsamples[s] > 0)
            (void) batch_rg_plan_append(b, who, s, nsamples[s], true);
    if (b->inc_rs) {
        /* (the same for the conversion: every stream's call checked and the round's list made large enough, then counted) */
        size_t  ntiles = 0;
        for (int s = 0; s < b->B; s++)
            if (nsamples[s] > 0 && (rc = batch_rs_plan_append(b, who, s, nsamples[s], false, &ntiles)) != 0)
                return rc;
        try {
            b->h_tiles.reserve(b->h_tiles.size() + ntiles);
        }
        catch(const std::bad_alloc &) {
            snprintf(g_err, sizeof(g_err), "%s: out of memory (tile table)", who);
            return LAMEHIP_ERR_DEVICE;
        }
        for (int s = 0; s < b->B; s++)
            if (nsamples[s] > 0 && (rc = batch_rs_plan_append(b, who, s, nsamples[s], true)) != 0)
                return rc;
    }
    bool const one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    for (int s = 0; s < b->B; s++) {
        if (nsamples[s] == 0)
            continue;
        LhApSeg & g = b->h_ap.get()[LH_STAGE_SEGS + nsegs++];
        g.l = (unsigned long long) ((uintptr_t) dev + (uintptr_t) ((long long) s * stream_stride * b->esz));
        g.r = one_plane ? g.l : g.l + (unsigned long long) (plane_stride * b->esz);
        g.at = b->fed[(size_t) s] + b->staged[(size_t) s];
        g.n = nsamples[s];
        g.stream = s;
        g.stride = stride;
        if (nsamples[s] > max_n)
            max_n = nsamples[s];
    }
    return batch_append_resident(b, nsegs, max_n);
}

/* HIP-event time of the append launches (lh_append_kernel) since, and including, the last lamehip_batch_encode_available /
 * _finish; not part of lamehip_batch_last_kernel_ms */
extern "C" float
lamehip_batch_last_append_ms(lamehip_batch * b)
{
    return b ? b->ap_ms : 0.0f;
}

/* frames of a stream that are complete once `fed' samples are in: frame f reads 1904 samples from
 * 1152 f - 528 on (reference lame.c:1737-1766) */
static int
frames_complete(long fed, const LhConfig & c)
{
    long const have = fed + LH_MF_START;
    return have >= mfn_of(c) ? (int) ((have - mfn_of(c)) / fs_of(c) + 1) : 0;
}

/* A batch that converts round by round: the tiles planned since the last round (lh_resample_tiles_kernel), ONE launch on
 * the batch's stream between ev_rs[0] and ev_rs[1], behind the append launches -- every chunk is in the input pool and
 * counted in fed[] -- and in front of the encode launch.  The list stays until the round's wait: it is read from here. */
static int
batch_tiles_launch(lamehip_batch * b)
{
    size_t const ntiles = b->h_tiles.size();
    b->rs_ran = 0;
    if (ntiles == 0)
        return 0;
    for (int s = 0; s < b->B; s++)
        b->h_rs_lens[(size_t) s] = b->fed[(size_t) s];
    /* (twice what is needed; drained first: nothing of an earlier round is in flight, a round ends with a wait) */
    HIPCHK(b->d_tiles.reserve(ntiles, ntiles + 1024, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_tiles.get(), b->h_tiles.data(), ntiles * sizeof(LhRsTile), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_rs_lens.get(), b->h_rs_lens.data(), (size_t) b->B * sizeof(long long), hipMemcpyHostToDevice, b->stream));
    LhRsParams p;
    memset(&p, 0, sizeof(p));
    p.ratio = b->rs->ratio;
    p.m = b->stype != LH_PCM_S16 ? lh_pcm_matrix(b->stype, b->cfg.pcm_scale, b->cfg.pcm_mix, b->cfg.pcm_scale_r)
        : lh_rs_matrix(b->cfg.pcm_scale, b->cfg.pcm_mix, b->cfg.pcm_scale_r);
    p.taps = b->rs->taps;
    p.phases = b->rs->phases;
    p.channels = b->cfg.channels;
    p.one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    p.cap_in = b->cap;
    p.cap_out = b->capf;
    /* (a round with a tile of another class than the batch's own: the mixed kernel) */
    bool    mixed = false;
    if (b->rs_ncls > 1)
        for (const LhRsTile & t:b->h_tiles)
            if (t.cls != 0) {
                mixed = true;
                break;
            }
    HIPCHK(hipEventRecord(b->ev_rs[0], b->stream));
    int const rc = mixed
        ? lh_launch_resample_mixed_tiles(b->stype, &p, b->d_rs_classes.get(), b->rs_ncls, b->d_rs_banks.get(), b->d_tiles.get(),
                                         (long long) ntiles, b->d_rs_lens.get(), b->d_pcm.get(), b->d_pcmf.get(),
                                         (void *) (hipStream_t) b->stream)
        : lh_launch_resample_tiles(b->stype, &p, b->d_rs_bank.get(), b->d_tiles.get(), (long long) ntiles, b->d_rs_lens.get(),
                                   b->d_pcm.get(), b->d_pcmf.get(), (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("conversion launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_rs[1], b->stream));
    b->rs_ran = 1;
    return 0;
}

/* behind the round's wait: the time of its tile launch (lamehip_batch_last_resample_ms), and the list is done with */
static void
batch_tiles_done(lamehip_batch * b)
{
    if (!b->inc_rs)
        return;
    b->rs_ms = 0;
    if (b->rs_ran && hipEventElapsedTime(&b->rs_ms, b->ev_rs[0], b->ev_rs[1]) != hipSuccess) {
        (void) hipGetLastError();
        b->rs_ms = 0;
    }
    b->h_tiles.clear();
    for (int s = 0; s < b->B; s++)
        b->rs_conv[(size_t) s] = b->rs_cur[(size_t) s].fed;
}

static int batch_gain_round(lamehip_batch * b);
static void batch_gain_round_done(lamehip_batch * b, int end);

/* behind the round's wait: the time of its encode launch (lamehip_batch_last_kernel_ms) */
static void
batch_round_time(lamehip_batch * b)
{
    float   ms = 0;
    if (hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess)
        b->last_ms = ms;
    else
        (void) hipGetLastError();
}

/* A round on the device packer, in front of its launches: what the drain needs -- every stream's bound (the frames done
 * after the round, each as large as the settings allow, less what has been handed out), the gather's tiles, room for the
 * table, the tiles and the round buffer in HBM and in pinned memory.  Allocates; a failure returns LAMEHIP_ERR_DEVICE with
 * nothing launched. */
static int
batch_drain_plan(lamehip_batch * b, const std::vector < int >&upto)
{
    b->dr_have = 0;             /* (the buffers may move; what has not been handed out is gathered again) */
    try {
        b->dr_bound.resize((size_t) b->B);
        for (int s = 0; s < b->B; s++) {
            int const frames = upto[(size_t) s] > b->done[(size_t) s] ? upto[(size_t) s] : b->done[(size_t) s];
            b->dr_bound[(size_t) s] = lh_drain_bound(b->dr_next[(size_t) s], frames - b->dr_done[(size_t) s], b->dr_frame_max, b->dr_slice,
                                                     b->dr_drained[(size_t) s]);
        }
        long long const ntiles = lh_drain_tiles(b->dr_bound.data(), b->B, nullptr, 0, &b->dr_padded);
        b->h_dr_tiles.resize((size_t) ntiles);
        (void) lh_drain_tiles(b->dr_bound.data(), b->B, b->h_dr_tiles.data(), ntiles, nullptr);
        b->dr_sent = b->dr_drained;
    }
    catch(const std::bad_alloc &) {
        snprintf(g_err, sizeof(g_err), "incremental packing: out of memory (drain plan)");
        return LAMEHIP_ERR_DEVICE;
    }
    /* (twice what is needed; drained first: nothing of an earlier round is in flight, a round ends with a wait.  The pinned
     * buffer may move: what lamehip_batch_drain_ptr handed out is valid until the next round) */
    size_t const room = (size_t) b->dr_padded + 64;
    HIPCHK(b->d_dr_tiles.reserve(b->h_dr_tiles.size() + 1, b->h_dr_tiles.size() + 1024, b->stream));
    HIPCHK(b->d_round.reserve(room, room, b->stream));
    HIPCHK(b->h_round.reserve(room, room, b->stream));
    return 0;
}

/* the info byte of the LAME extension for a stream that arrives at rate_in: lh_tag_template's, made as the batch's own
 * template is (lamehip_batch_set_incremental_tagging) with that source rate */
static int
batch_tag_info(const lamehip_batch * b, int rate_in)
{
    unsigned char frame[2880]; /* (lh_tag_init allows no larger frame) */
    LhVbrTag v;
    int const total = lh_tag_init(&v, &b->cfg);
    if (total <= 0 || total > (int) sizeof(frame))
        return 0;
    v.samplerate_in = rate_in;
    lh_tag_template(&v, &b->cfg, b->cfg.vbr_q, frame);
    return frame[b->tg_p.at + LH_TAG_AT_EXT + LH_TAG_EXT_INFO];
}

/* A round's tag launch (lamehip_batch_set_incremental_tagging), behind the drain's launches -- its table in HBM says which
 * bytes are final -- between ev_tg[0] and ev_tg[1].  The final round brings what the kernel cannot know, every stream's end
 * padding: the figure the one-shot tagged path uses for a stream of that many samples, or the conversion's -- and with it
 * the info byte of a stream at an input rate of its own (lh_tag.h: lh_tag_pad_with_info). */
static int
batch_tag_launch(lamehip_batch * b, int end, int nending)
{
    b->tg_ran = 0;
    if (!b->inc_tag || b->tg_p.total <= 0)
        return 0;
    if (nending > 0) {
        /* (the streams that end in this round: the kernel reads no other's) */
        for (int s = 0; s < b->B; s++)
            if (b->ending[(size_t) s]) {
                b->h_tg_pad[(size_t) s] = batch_padding(b, s);
                /* (a stream at an input rate of its own: its info byte, which the template has for the batch's rate) */
                if (batch_stream_cls(b, s) != 0)
                    b->h_tg_pad[(size_t) s] = lh_tag_pad_with_info(b->h_tg_pad[(size_t) s], batch_tag_info(b, batch_stream_rs(b, s)->rate_in));
            }
        HIPCHK(hipMemcpyAsync(b->d_tg_pad.get(), b->h_tg_pad.data(), (size_t) b->B * sizeof(int), hipMemcpyHostToDevice, b->stream));
    }
    HIPCHK(hipEventRecord(b->ev_tg[0], b->stream));
    int const rc = lh_launch_tag_resume(&b->tg_p, b->d_tg_pow.get(), (const LhStreamDesc *) b->d_stage.get(), b->d_state.get(),
                                        b->d_dr_rows.get(), b->d_out.get(), b->d_bytes.get(), b->d_tg_tmpl.get(), b->d_tg_pad.get(),
                                        b->d_tg_carry.get(), b->d_tg_tags.get(), end, b->B, (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("tag launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_tg[1], b->stream));
    b->tg_ran = 1;
    return 0;
}

/* ... and behind its encode launch: the table of tiles and `drained' to HBM, the three drain launches between ev_dr[0] and
 * ev_dr[1], the tag launch of a batch that carries tag frames, and the table on its way home -- behind it, in the final
 * round, the tag frames */
static int
batch_drain_launch(lamehip_batch * b, int end)
{
    LhDrainParams p;
    int     nending = 0;
    for (int s = 0; s < b->B; s++)
        nending += b->ending[(size_t) s] != 0;
    /* (the kernels take "behind the flush" from every stream's descriptor; the scalar says the same of all streams at once, in
     * the round that ends them all) */
    end = end && nending == b->B;
    memset(&p, 0, sizeof(p));
    p.sideinfo_len = b->cfg.sideinfo_len;
    p.frame_factor = (b->cfg.version + 1) * 72000;
    p.samplerate = b->cfg.samplerate;
    p.final = end;
    for (int i = 0; i < 16; i++)
        p.kbps[i] = (int16_t) ((i > 0 && i < 15) ? lh_tag_kbps(b->cfg.version, i) : 0);
    b->dr_have = 0;
    if (!b->h_dr_tiles.empty())
        HIPCHK(hipMemcpyAsync(b->d_dr_tiles.get(), b->h_dr_tiles.data(), b->h_dr_tiles.size() * sizeof(LhDrainTile), hipMemcpyHostToDevice,
                              b->stream));
    HIPCHK(hipMemcpyAsync(b->d_dr_drained.get(), b->dr_sent.data(), (size_t) b->B * sizeof(long long), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipEventRecord(b->ev_dr[0], b->stream));
    int const rc = lh_launch_drain(&p, (const LhStreamDesc *) b->d_stage.get(), b->d_state.get(), b->d_dr_drained.get(), b->d_dr_carry.get(),
                                   b->d_bytes.get(), b->d_dr_rows.get(), b->B, b->d_dr_tiles.get(), (long long) b->h_dr_tiles.size(),
                                   b->d_round.get(), (long long) b->d_round.cap(), (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("drain launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_dr[1], b->stream));
    b->dr_ran = 1;
    {
        int const tr = batch_tag_launch(b, end, nending);
        if (tr)
            return tr;
    }
    HIPCHK(hipMemcpyAsync(b->h_dr_rows.get(), b->d_dr_rows.get(), ((size_t) b->B + 1) * sizeof(LhDrainRow), hipMemcpyDeviceToHost, b->stream));
    if (nending > 0 && b->tg_ran) {
        /* (all streams end: straight to where the getters read; some: the array stops over in a buffer of its own, and the
         * ending streams' frames alone move on behind the round's wait -- a frame handed out earlier, its gain patched in,
         * stays as it is) */
        size_t const room = (size_t) b->B * (size_t) b->tg_p.total;
        unsigned char *to = b->h_tg_tags.get();
        if (nending < b->B) {
            if (!b->h_tg_round.get() && b->h_tg_round.alloc(room) != hipSuccess)
                return set_err("tag frames: pinned allocation", hipGetLastError());
            to = b->h_tg_round.get();
        }
        HIPCHK(hipMemcpyAsync(to, b->d_tg_tags.get(), room, hipMemcpyDeviceToHost, b->stream));
    }
    return 0;
}

/* ... and the way home: behind the table (the caller has waited for it) ONE copy of exactly the round's bytes, then the
 * round's wait.  A stream whose packer reported a status -- or whose position the drain could not place in its slice --
 * fails the round with LAMEHIP_ERR_PAYLOAD; the other streams' bytes are there. */
static int
batch_drain_home(lamehip_batch * b, int end)
{
    const LhDrainRow *rows = b->h_dr_rows.get();
    long long const total = rows[b->B].off;
    b->dr_ms = 0;
    if (b->dr_ran && hipEventElapsedTime(&b->dr_ms, b->ev_dr[0], b->ev_dr[1]) != hipSuccess) {
        (void) hipGetLastError();
        b->dr_ms = 0;
    }
    if (b->inc_tag) {
        /* (the tag launch's time; the final round's frames came home behind the table, which the caller has waited for) */
        b->tag_ms = 0;
        if (b->tg_ran && hipEventElapsedTime(&b->tag_ms, b->ev_tg[0], b->ev_tg[1]) != hipSuccess) {
            (void) hipGetLastError();
            b->tag_ms = 0;
        }
        if (b->tg_ran) {
            int     nending = 0;
            for (int s = 0; s < b->B; s++)
                nending += b->ending[(size_t) s] != 0;
            for (int s = 0; s < b->B && nending > 0; s++) {
                if (!b->ending[(size_t) s])
                    continue;
                size_t const at = (size_t) s * (size_t) b->tg_p.total;
                if (nending < b->B)
                    memcpy(b->h_tg_tags.get() + at, b->h_tg_round.get() + at, (size_t) b->tg_p.total);
                b->tg_has[(size_t) s] = 1;
                b->tg_patched[(size_t) s] = 0;
                b->tg_have = 1;
            }
        }
    }
    if (total < 0 || total > b->dr_padded) {
        snprintf(g_err, sizeof(g_err), "incremental packing: the drain found %lld bytes where the round's bound is %lld", total, b->dr_padded);
        return LAMEHIP_ERR_PAYLOAD;
    }
    for (int s = 0; s < b->B; s++)
        if (rows[s].n < 0 || rows[s].n > b->dr_bound[(size_t) s] || rows[s].off < 0 || rows[s].off + rows[s].n > total) {
            snprintf(g_err, sizeof(g_err), "incremental packing: the drain found %lld bytes of stream %d where its bound is %lld", rows[s].n, s,
                     b->dr_bound[(size_t) s]);
            return LAMEHIP_ERR_PAYLOAD;
        }
    if (total > 0) {
        HIPCHK(hipMemcpyAsync(b->h_round.get(), b->d_round.get(), (size_t) total, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    b->dr_have = 1;
    return 0;
}

/* ... and the books: where every stream's frames end now (the next round's bounds start there), and the streams' statuses */
static int
batch_drain_done(lamehip_batch * b, const std::vector < int >&upto)
{
    const LhDrainRow *rows = b->h_dr_rows.get();
    for (int s = 0; s < b->B; s++) {
        b->dr_next[(size_t) s] = rows[s].next;
        b->dr_done[(size_t) s] = upto[(size_t) s] > b->done[(size_t) s] ? upto[(size_t) s] : b->done[(size_t) s];
    }
    for (int s = 0; s < b->B; s++)
        if (rows[s].status != 0) {
            snprintf(g_err, sizeof(g_err), "device bit packer reported status %d for stream %d", rows[s].status, s);
            return LAMEHIP_ERR_PAYLOAD;
        }
    return 0;
}

/* The slots restarted since the last round: ONE launch of lh_slot_restart_kernel on the batch's stream, between ev_sl[0] and
 * ev_sl[1], puts their records in HBM back -- in front of everything that reads them: the round's launches, which call this
 * first, and lamehip_batch_get_state. */
static int
batch_restart_launch(lamehip_batch * b)
{
    size_t const n = b->sl_list.size();
    if (n == 0)
        return 0;
    if (!b->ev_sl[0] && (b->ev_sl[0].create() != hipSuccess || b->ev_sl[1].create() != hipSuccess))
        return set_err("hipEventCreate", hipGetLastError());
    if (!b->d_sl_list.get())
        HIPCHK(b->d_sl_list.alloc((size_t) b->B));
    /* (the copy reads the list it is given until the stream has been waited for: the gap's list changes places with the one
     * of the launch before, which a wait lies behind) */
    b->sl_sent.swap(b->sl_list);
    b->sl_list.clear();
    HIPCHK(hipMemcpyAsync(b->d_sl_list.get(), b->sl_sent.data(), n * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipEventRecord(b->ev_sl[0], b->stream));
    int const rc = lh_launch_slot_restart(b->d_sl_list.get(), (int) n, b->B, b->d_state.get(), b->d_state0.get(),
                                          b->inc_pack ? b->d_dr_carry.get() : nullptr, b->inc_tag ? b->d_tg_carry.get() : nullptr,
                                          b->inc_rg ? b->d_rg_carry.get() : nullptr, (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("slot restart launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_sl[1], b->stream));
    b->sl_ran = 1;
    return 0;
}

/* behind a wait for the batch's stream: the time of the restart launch (lamehip_batch_last_restart_ms) */
static void
batch_restart_time(lamehip_batch * b)
{
    if (!b->sl_ran)
        return;
    b->sl_ran = 0;
    b->sl_ms = 0;
    if (hipEventElapsedTime(&b->sl_ms, b->ev_sl[0], b->ev_sl[1]) != hipSuccess) {
        (void) hipGetLastError();
        b->sl_ms = 0;
    }
}

/* at the head of a round: the gap's restart launch, if one is owed; the figure of lamehip_batch_last_restart_ms is this gap's */
static int
batch_restart_round(lamehip_batch * b)
{
    if (!b->sl_gap)
        b->sl_ms = 0;
    b->sl_gap = 0;
    return batch_restart_launch(b);
}

/* behind a round's wait: the streams the round flushed have ended -- on the host packer with the stuffing that completes
 * their last frame (lh_bs_flush) */
static void
batch_round_close(lamehip_batch * b)
{
    batch_restart_time(b);
    for (int s = 0; s < b->B; s++) {
        if (!b->ending[(size_t) s])
            continue;
        if (!b->inc_pack) {
            LhBitstream *bs = &b->packer[(size_t) s];
            std::vector < unsigned char >&out = b->pending[(size_t) s];
            size_t const at = out.size();
            lh_bs_flush(bs, &b->cfg, b->have_last[(size_t) s] ? &b->last[(size_t) s] : nullptr);
            out.resize(at + (size_t) lh_bs_pending(bs));
            int const k = lh_bs_copy(bs, out.data() + at, 0);
            out.resize(at + (size_t) (k > 0 ? k : 0));
        }
        b->ending[(size_t) s] = 0;
        b->slot[(size_t) s] = (char) LH_SLOT_ENDED;
    }
}

/* encode frames [done, upto[s]) of every stream and pack them into pending[]; ending[s] marks the streams whose last frames
 * these are (flush); `end': the round closes the batch */
static int
batch_encode_range(lamehip_batch * b, const std::vector < int >&upto, int end)
{
    LhStreamDesc *descs = (LhStreamDesc *) b->h_stage.get();
    long long total = 0;
    int     rc;
    if ((rc = batch_restart_round(b)) != 0)
        return rc;
    /* (a batch that converts: the kernels read the float pool's rows, as far as the conversion has come) */
    long long const row = b->inc_rs ? b->capf : b->cap;
    for (int s = 0; s < b->B; s++) {
        LhStreamDesc & d = descs[s];
        int const nf = upto[(size_t) s] - b->done[(size_t) s];
        memset(&d, 0, sizeof(d));
        d.pcm_l = ((long long) s * 2) * row;
        d.pcm_r = ((long long) s * 2 + 1) * row;
        d.pcm_base = 0;
        d.nsamples = b->inc_rs ? (long) b->rs_cur[(size_t) s].fed : b->fed[(size_t) s] + b->staged[(size_t) s];
        d.out_index = total;
        d.frame_begin = b->done[(size_t) s];
        d.frame_end = upto[(size_t) s];
        /* (a stream that ends in this round; a slot whose stream ended in an earlier one keeps the flag, with no frames: the
         * encode kernels have nothing to do for it, the drain goes on finding its last frame's end) */
        d.flush = b->ending[(size_t) s] || b->slot[(size_t) s] == LH_SLOT_ENDED;
        if (b->inc_pack) {
            /* (the device packer: the stream's slice, the same in every round) */
            d.bytes_base = b->bytes_off[(size_t) s];
            d.bytes_cap = b->dr_slice;
        }
        total += nf > 0 ? nf : 0;
    }
    HIPCHK(b->d_out.reserve((size_t) total, 1024));
    if (b->inc_pack && total > 0 && (rc = batch_drain_plan(b, upto)) != 0)
        return rc;
    /* descriptors, then what is staged (chunk table + the arena's bytes in use), then the scatter */
    HIPCHK(hipMemcpyAsync(b->d_stage.get(), b->h_stage.get(), (size_t) b->B * sizeof(LhStreamDesc), hipMemcpyHostToDevice, b->stream));
    if ((rc = batch_stage_flush(b, 0)) != 0)
        return rc;
    /* (the round's conversion, also when no frame is complete yet: the floats are there when one is) */
    if (b->inc_rs && (rc = batch_tiles_launch(b)) != 0)
        return rc;
    /* (the round's ReplayGain analysis: behind them, the samples are in the pool the kernels read) */
    if (b->inc_rg && (rc = batch_gain_round(b)) != 0)
        return rc;
    if (total == 0) {
        b->st_ran = b->st_timed = 0;    /* (no statistics launch: the tables stay what they are) */
        b->st_ms = 0;
        b->dr_ms = 0;           /* (no drain either: what the last round brought home stays where it is) */
        if (b->inc_tag) {
            b->tg_ran = 0;      /* (and no tag launch) */
            b->tag_ms = 0;
        }
        HIPCHK(hipStreamSynchronize(b->stream));
        batch_append_time(b);
        batch_tiles_done(b);
        batch_gain_round_done(b, end);
        batch_round_close(b);
        return 0;
    }
    {
        /* (a typed batch: the kernels read the float pool the appends filled) */
        LhLaunchPlan plan;
        if ((rc = batch_plan(b, descs, &plan)) != 0
            || (rc = batch_launch(b, batch_reads_floats(b) ? (const int16_t *) 0 : b->d_pcm.get(),
                                  batch_reads_floats(b) ? b->d_pcmf.get() : (const float *) 0, (const LhStreamDesc *) b->d_stage.get(), plan,
                                  b->inc_pack ? b->d_bytes.get() : (uint8_t *) 0)) != 0)
            return rc;
    }
    b->launched = 1;
    if (b->inc_pack) {
        /* the device packer: no record comes home and no host packer runs -- the drain kernels behind the encode launch, their
         * table, the round's bytes in one copy (the emit stage has read its records in d_out on the device) */
        if ((rc = batch_drain_launch(b, end)) != 0)
            return rc;
        HIPCHK(hipStreamSynchronize(b->stream));
        batch_round_time(b);
        batch_append_time(b);
        batch_tiles_done(b);
        batch_gain_round_done(b, end);
        if ((rc = batch_drain_home(b, end)) == 0)
            rc = batch_drain_done(b, upto);
        for (int s = 0; s < b->B; s++)
            if (upto[(size_t) s] > b->done[(size_t) s])
                b->done[(size_t) s] = upto[(size_t) s];
        batch_round_close(b);
        return rc ? rc : (int) total;
    }
    b->h_new.resize((size_t) total);
    HIPCHK(hipMemcpyAsync(b->h_new.data(), b->d_out.get(), (size_t) total * sizeof(LhFrameOut), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    batch_round_time(b);
    batch_append_time(b);
    batch_tiles_done(b);
    batch_gain_round_done(b, end);
    for (int s = 0; s < b->B; s++) {
        LhBitstream *bs = &b->packer[(size_t) s];
        std::vector < unsigned char >&out = b->pending[(size_t) s];
        for (int f = b->done[(size_t) s]; f < upto[(size_t) s]; f++) {
            const LhFrameOut & fo = b->h_new[(size_t) (descs[s].out_index + (f - descs[s].frame_begin))];
            size_t  at;
            int     k;
            if (lh_bs_format_frame(bs, &b->cfg, b->tab, &fo) != 0) {
                snprintf(g_err, sizeof(g_err), "inconsistent device payload (packer check %d) stream %d frame %d", bs->error, s, f);
                return LAMEHIP_ERR_PAYLOAD;
            }
            at = out.size();
            out.resize(at + (size_t) lh_bs_pending(bs));
            k = lh_bs_copy(bs, out.data() + at, 0);
            out.resize(at + (size_t) (k > 0 ? k : 0));
            b->last[(size_t) s] = fo;
            b->have_last[(size_t) s] = 1;
        }
        if (upto[(size_t) s] > b->done[(size_t) s])
            b->done[(size_t) s] = upto[(size_t) s];
    }
    batch_round_close(b);
    return (int) total;
}

static int batch_rs_plan_finish(lamehip_batch * b);
static int batch_rg_plan_finish(lamehip_batch * b);

/* One round: the frames that became complete of the streams that go on, the flush of those that end with it -- the ones
 * lamehip_batch_end_stream named, and with `end' (lamehip_batch_finish) every stream that has not ended --, nothing of those
 * that ended in an earlier round.  who: the entry point, for the messages. */
static int
batch_round(lamehip_batch * b, const char *who, int end)
{
    std::vector < int >upto;
    int     rc, nending = 0;
    if ((rc = batch_incremental_begin(b, who, 0)) != 0)
        return rc;
    if ((rc = batch_stage_reserve(b)) != 0)
        return rc;
    batch_append_time(b);
    b->ap_ms = 0;               /* (lamehip_batch_last_append_ms counts from here) */
    upto.resize((size_t) b->B);
    for (int s = 0; s < b->B; s++) {
        b->ending[(size_t) s] = b->slot[(size_t) s] == LH_SLOT_ENDING || (end && b->slot[(size_t) s] == LH_SLOT_LIVE);
        nending += b->ending[(size_t) s] != 0;
    }
    if (end && nending == 0) {
        /* (every stream has ended on its own: nothing to encode, the batch closes) */
        b->finished = 1;
        return 0;
    }
    if (nending > 0 && b->inc_rs && (rc = batch_rs_plan_finish(b)) != 0)
        return rc;
    if (nending > 0 && b->inc_rg && !b->inc_rs && (rc = batch_rg_plan_finish(b)) != 0)
        return rc;
    for (int s = 0; s < b->B; s++) {
        if (b->slot[(size_t) s] == LH_SLOT_ENDED)
            upto[(size_t) s] = b->done[(size_t) s];
        else if (b->ending[(size_t) s]) {
            if (!b->inc_rs) {
                long const len = b->fed[(size_t) s] + b->staged[(size_t) s];
                b->len[(size_t) s] = len;
                b->nframes[(size_t) s] = lh_total_frames_fs(len, fs_of(b->cfg));
            }
            upto[(size_t) s] = b->nframes[(size_t) s];
        }
        else
            upto[(size_t) s] = frames_complete(b->inc_rs ? (long) b->rs_cur[(size_t) s].fed : b->fed[(size_t) s] + b->staged[(size_t) s], b->cfg);
    }
    if (b->inc_pack)
        for (int s = 0; s < b->B; s++)
            if (b->ending[(size_t) s] && upto[(size_t) s] <= b->done[(size_t) s]) {
                /* (the kernel's flush -- the stuffing that completes the last frame -- goes with a stream's last frame:
                 * lh_total_frames_fs leaves every stream at least one for this round, whatever was fed) */
                snprintf(g_err, sizeof(g_err), "%s: stream %d has no frame left for the flush (%d encoded, %d in all)", who, s,
                         b->done[(size_t) s], upto[(size_t) s]);
                return -1;
            }
    int const n = batch_encode_range(b, upto, end);
    if (n >= 0 && end)
        b->finished = 1;
    return n;
}

extern "C" int
lamehip_batch_encode_available(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->finished) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_encode_available: the batch is finished (lamehip_batch_reset starts it over)");
        return -1;
    }
    if (batch_refuse_gain(b, "lamehip_batch_encode_available"))
        return -1;
    return batch_round(b, "lamehip_batch_encode_available", 0);
}

/* A batch that converts round by round, at the end of the streams the round ends (ending[]): every such stream's flush
 * planned from its cursor (lh_rs_plan_flush) -- its
 * tiles join the round's list, its converted length, frame count and end padding are the plan's.  Every append made sure
 * the flush fits the float pool.  An allocation failure returns LAMEHIP_ERR_DEVICE with the batch as it was. */
static int
batch_rs_plan_finish(lamehip_batch * b)
{
    int const fs = fs_of(b->cfg), mfn = mfn_of(b->cfg);
    size_t const tiles_before = b->h_tiles.size();
    std::vector < LhRsCursor > end;
    std::vector < int >padding;
    std::vector < size_t > rg_before;   /* (ReplayGain round by round: the flush's made counts join the last round's blocks) */
    try {
        end = b->rs_cur;
        padding.assign((size_t) b->B, 0);
        for (const std::vector < int >&g:b->rg_blk)
            rg_before.push_back(g.size());
        for (int s = 0; s < b->B; s++) {
            if (!b->ending[(size_t) s])
                continue;
            const LhResampler *const rs = batch_stream_rs(b, s);
            int const cls = batch_stream_cls(b, s);
            LhRsCursor c = b->rs_cur[(size_t) s];
            int const nblk = lh_rs_plan_flush(rs, fs, mfn, &c, nullptr, 0, &padding[(size_t) s]);
            b->rs_blk.resize((size_t) nblk);
            (void) lh_rs_plan_flush(rs, fs, mfn, &end[(size_t) s], b->rs_blk.data(), nblk, &padding[(size_t) s]);
            for (const LhRsBlock & k:b->rs_blk)
                if (b->inc_rg && k.made > 0)
                    b->rg_blk[(size_t) s].push_back(k.made);
            for (const LhRsBlock & k:b->rs_blk) {
                size_t const at = b->h_tiles.size();
                b->h_tiles.resize(at + (size_t) lh_rs_block_tiles_class(rs, &k, s, cls, nullptr, 0));
                (void) lh_rs_block_tiles_class(rs, &k, s, cls, b->h_tiles.data() + at, (int) (b->h_tiles.size() - at));
            }
        }
    }
    catch(const std::bad_alloc &) {
        b->h_tiles.resize(tiles_before);
        for (size_t s = 0; s < rg_before.size(); s++)
            b->rg_blk[s].resize(rg_before[s]);
        snprintf(g_err, sizeof(g_err), "lamehip_batch_finish: out of memory (conversion plan)");
        return LAMEHIP_ERR_DEVICE;
    }
    for (int s = 0; s < b->B; s++) {
        if (!b->ending[(size_t) s])
            continue;
        b->rs_cur[(size_t) s] = end[(size_t) s];
        b->len_in[(size_t) s] = b->fed[(size_t) s] + b->staged[(size_t) s];
        b->len[(size_t) s] = (long) end[(size_t) s].fed;
        b->nframes[(size_t) s] = end[(size_t) s].frames;
        b->padding[(size_t) s] = padding[(size_t) s];
    }
    return 0;
}

/* A batch that measures ReplayGain round by round and does not convert, at the end of the streams the round ends (ending[]):
 * every such stream's flush as the analysis
 * hears it (lh_gain_plan_flush from the stream's cursor) joins the last round's blocks.  Every append made sure it is not too
 * long.  An allocation failure returns LAMEHIP_ERR_DEVICE with the batch as it was. */
static int
batch_rg_plan_finish(lamehip_batch * b)
{
    int const fs = fs_of(b->cfg), mfn = mfn_of(b->cfg);
    try {
        for (int s = 0; s < b->B; s++) {
            if (!b->ending[(size_t) s])
                continue;
            LhGainCursor c = b->rg_cur[(size_t) s];
            std::vector < int >&g = b->rg_blk[(size_t) s];
            g.reserve(g.size() + (size_t) lh_gain_plan_flush(&c, fs, mfn, nullptr, 0));
        }
    }
    catch(const std::bad_alloc &) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_finish: out of memory (gain plan)");
        return LAMEHIP_ERR_DEVICE;
    }
    for (int s = 0; s < b->B; s++) {
        if (!b->ending[(size_t) s])
            continue;
        LhGainCursor c = b->rg_cur[(size_t) s];
        std::vector < int >&g = b->rg_blk[(size_t) s];
        size_t const at = g.size();
        int const nblk = lh_gain_plan_flush(&c, fs, mfn, nullptr, 0);
        g.resize(at + (size_t) nblk);
        (void) lh_gain_plan_flush(&b->rg_cur[(size_t) s], fs, mfn, g.data() + at, nblk);
    }
    return 0;
}

/* lame_encode_flush for every stream of an incremental batch that has not ended on its own (lamehip_batch_end_stream):
 * the frames still owed for the samples fed (with the reference's end padding), then the stuffing that completes the last
 * frame; the streams that have ended stay as they are, and the batch is closed */
extern "C" int
lamehip_batch_finish(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->finished) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_finish: the batch is finished already (lamehip_batch_reset starts it over)");
        return -1;
    }
    if (batch_refuse_gain(b, "lamehip_batch_finish"))
        return -1;
    return batch_round(b, "lamehip_batch_finish", 1);
}

/* ---- the batch as a pool of slots: streams that end and begin on their own ---- */

/* what the two calls check first: 0, or the call's return value */
static int
batch_slot_enter(lamehip_batch * b, const char *who, int s)
{
    if (!b || s < 0 || s >= b->B) {
        snprintf(g_err, sizeof(g_err), "%s: no such stream", who);
        return -1;
    }
    if (b->finished) {
        snprintf(g_err, sizeof(g_err), "%s: the batch is finished (lamehip_batch_reset starts it over)", who);
        return -1;
    }
    return 0;
}

/* lame_encode_flush for stream s alone, carried out by the next lamehip_batch_encode_available (or lamehip_batch_finish):
 * nothing is launched here */
extern "C" int
lamehip_batch_end_stream(lamehip_batch * b, int s)
{
    static const char who[] = "lamehip_batch_end_stream";
    LhDeviceScope const on_device(b ? b->device : -1);
    int     rc;
    if ((rc = batch_slot_enter(b, who, s)) != 0)
        return rc;
    if (batch_refuse_gain(b, who))
        return -1;
    if ((rc = batch_incremental_begin(b, who, 0)) != 0)
        return rc;
    if (b->slot[(size_t) s] != LH_SLOT_LIVE) {
        snprintf(g_err, sizeof(g_err), "%s: stream %d %s", who, s,
                 b->slot[(size_t) s] == LH_SLOT_ENDING ? "ends with the next round already" : "has ended already (lamehip_batch_restart_stream "
                 "gives its slot to the next stream)");
        return -1;
    }
    b->slot[(size_t) s] = (char) LH_SLOT_ENDING;
    return 0;
}

extern "C" int
lamehip_batch_stream_ended(lamehip_batch * b, int s)
{
    if (!b || s < 0 || s >= b->B)
        return -1;
    return !b->slot.empty() && b->slot[(size_t) s] == LH_SLOT_ENDED;
}

/* the slot of stream s, which has ended and whose bytes have been handed out, takes a new stream: the host's books of the
 * slot in front of the first sample here, its records in HBM with the restart launch at the head of the next round */
extern "C" int
lamehip_batch_restart_stream(lamehip_batch * b, int s)
{
    static const char who[] = "lamehip_batch_restart_stream";
    LhDeviceScope const on_device(b ? b->device : -1);
    int     rc;
    if ((rc = batch_slot_enter(b, who, s)) != 0)
        return rc;
    if (!b->incremental || b->slot[(size_t) s] != LH_SLOT_ENDED) {
        snprintf(g_err, sizeof(g_err), "%s: stream %d has not ended (lamehip_batch_end_stream, then a round: lamehip_batch_encode_available)",
                 who, s);
        return -1;
    }
    {
        long long left = 0;
        if (!b->inc_pack)
            left = (long long) b->pending[(size_t) s].size();
        else if (b->h_dr_rows.get()[s].status == 0)
            left = b->dr_next[(size_t) s] - b->dr_drained[(size_t) s];
        if (left > 0) {
            snprintf(g_err, sizeof(g_err), "%s: stream %d has %lld bytes that have not been handed out (lamehip_batch_drain)", who, s, left);
            return -1;
        }
    }
    /* everything that can fail first: a failure leaves the slot as it was */
    {
        LhBitstream fresh;
        try {
            b->sl_list.reserve((size_t) b->B);
        }
        catch(const std::bad_alloc &) {
            snprintf(g_err, sizeof(g_err), "%s: out of memory", who);
            return LAMEHIP_ERR_DEVICE;
        }
        if (lh_bs_init_sized(&fresh, 65536) != 0)
            return -2;
        /* (statistics: the slot's table alone goes back to zero, on the batch's stream, which the last round has left idle) */
        if (batch_stats_zero(b, s) != 0) {
            lh_bs_free(&fresh);
            return LAMEHIP_ERR_DEVICE;
        }
        lh_bs_free(&b->packer[(size_t) s]);
        b->packer[(size_t) s] = fresh;
    }
    b->pending[(size_t) s].clear();
    b->handed[(size_t) s].clear();
    b->fed[(size_t) s] = 0;
    b->done[(size_t) s] = 0;
    b->staged[(size_t) s] = 0;
    b->have_last[(size_t) s] = 0;
    b->len[(size_t) s] = 0;
    b->nframes[(size_t) s] = 0;
    b->padding[(size_t) s] = 0;
    if (b->inc_rs) {
        /* (the converter back in front of the first sample) */
        lh_rs_cursor_init(&b->rs_cur[(size_t) s]);
        b->rs_conv[(size_t) s] = 0;
        b->len_in[(size_t) s] = 0;
        /* (... and at the batch's own rate: the slot's next tenant states its rate again) */
        if (!b->rs_scls.empty())
            b->rs_scls[(size_t) s] = 0;
    }
    if (b->inc_rg) {
        /* (the analysis likewise: no window, no gain) */
        lh_gain_cursor_init(&b->rg_cur[(size_t) s]);
        b->rg_blk[(size_t) s].clear();
        b->rg_heard[(size_t) s] = 0;
        b->rg_win[(size_t) s].clear();
        b->rg_tenths[(size_t) s] = 0;
        b->rg_final[(size_t) s] = 0;
    }
    if (b->inc_pack) {
        /* (nothing handed out, the slice reused from its first byte; the round's table has nothing of the slot any more) */
        b->dr_drained[(size_t) s] = 0;
        b->dr_next[(size_t) s] = 0;
        b->dr_done[(size_t) s] = 0;
        if (b->h_dr_rows.get()) {
            b->h_dr_rows.get()[s].n = 0;
            b->h_dr_rows.get()[s].status = 0;
        }
    }
    if (b->inc_tag) {
        b->tg_has[(size_t) s] = 0;
        b->tg_patched[(size_t) s] = 0;
    }
    b->slot[(size_t) s] = (char) LH_SLOT_LIVE;
    b->sl_list.push_back(s);    /* (room was made above) */
    return 0;
}

/* HIP-event time of the restart launch (lh_slot_restart_kernel) in front of the last lamehip_batch_encode_available /
 * _finish; 0 when no slot was restarted in the gap before it.  Not part of lamehip_batch_last_kernel_ms. */
extern "C" float
lamehip_batch_last_restart_ms(lamehip_batch * b)
{
    return b ? b->sl_ms : 0.0f;
}

/* Statistics: the reference's five tables per stream (updateStats), counted on the device behind every encode launch.
 * Off by default; on any kind of batch, only before any PCM is handed over.  on = 0 puts the batch back as it was. */
extern "C" int
lamehip_batch_set_statistics(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->pcm_given || b->encoded || b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_statistics: only before any PCM is handed over");
        return -1;
    }
    if (!on || b->st_on) {
        b->st_on = on != 0 && b->st_on;
        return 0;
    }
    /* everything new first: a failure leaves the batch as it was */
    LhDevBuf < LhStatCarry > carry;
    LhEvent ev[2];
    std::vector < LhStatCarry > home;
    hipError_t e = carry.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = ev[0].create();
    if (e == hipSuccess)
        e = ev[1].create();
    if (e == hipSuccess)
        e = hipMemset(carry.get(), 0, (size_t) b->B * sizeof(LhStatCarry));
    if (e != hipSuccess)
        return set_err("lamehip_batch_set_statistics", e);
    try {
        home.resize((size_t) b->B);
    }
    catch(const std::bad_alloc &) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_statistics: out of memory");
        return LAMEHIP_ERR_DEVICE;
    }
    b->d_st_carry = std::move(carry);
    b->ev_st[0] = std::move(ev[0]);
    b->ev_st[1] = std::move(ev[1]);
    b->h_st = std::move(home);
    b->st_have = 0;
    b->st_ran = b->st_timed = 0;
    b->st_ms = 0;
    b->st_on = 1;
    return 0;
}

/* HIP-event time in ms of the statistics launch behind the last encode launch; 0 when none was launched (the switch off, a
 * round without frames).  Not part of lamehip_batch_last_kernel_ms.  Waits for the launch. */
extern "C" float
lamehip_batch_last_stats_ms(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b || !b->st_on || !b->st_ran)
        return 0.0f;
    if (!b->st_timed) {
        b->st_ms = 0;
        if (hipEventSynchronize(b->ev_st[1]) != hipSuccess || hipEventElapsedTime(&b->st_ms, b->ev_st[0], b->ev_st[1]) != hipSuccess) {
            (void) hipGetLastError();
            b->st_ms = 0;
        }
        b->st_timed = 1;
    }
    return b->st_ms;
}

/* the getters' way in: the switch, the stream index (s < 0 with all = true: every stream), and the tables at home -- the
 * whole array in one copy behind whatever the batch's stream still runs, on first use after a launch */
static int
batch_stats_ready(lamehip_batch * b, const char *who, int s, bool all = false)
{
    if (!b)
        return -1;
    if (!b->st_on) {
        snprintf(g_err, sizeof(g_err), "%s: the batch keeps no statistics (lamehip_batch_set_statistics)", who);
        return -1;
    }
    if (!all && (s < 0 || s >= b->B)) {
        snprintf(g_err, sizeof(g_err), "%s: no stream %d (the batch has %d)", who, s, b->B);
        return -1;
    }
    if (!b->st_have) {
        HIPCHK(hipMemcpyAsync(b->h_st.data(), b->d_st_carry.get(), (size_t) b->B * sizeof(LhStatCarry), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        b->st_have = 1;
    }
    return 0;
}

/* stream s's two tables as they stand behind the last launch: mode[bitrate index | 15 = all][mode extension | 4 = frames],
 * block[bitrate index | 15 = all][block type 0..3 | 4 = mixed | 5 = granules] (either may be null) */
extern "C" int
lamehip_batch_get_statistics(lamehip_batch * b, int s, int mode[16][5], int block[16][6])
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_stats_ready(b, "lamehip_batch_get_statistics", s);
    if (rc)
        return rc;
    if (mode)
        memcpy(mode, b->h_st[(size_t) s].mode, sizeof(b->h_st[0].mode));
    if (block)
        memcpy(block, b->h_st[(size_t) s].block, sizeof(b->h_st[0].block));
    return 0;
}

/* every stream's: out holds B x 176 ints, a stream's `mode' then its `block' */
extern "C" int
lamehip_batch_get_statistics_all(lamehip_batch * b, int *out)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_stats_ready(b, "lamehip_batch_get_statistics_all", -1, true);
    if (rc)
        return rc;
    if (!out) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_get_statistics_all: no room given");
        return -1;
    }
    memcpy(out, b->h_st.data(), (size_t) b->B * sizeof(LhStatCarry));
    return 0;
}

/* the reference's getters (lame_bitrate_hist and so on), per stream */
extern "C" int
lamehip_batch_bitrate_hist(lamehip_batch * b, int s, int bitrate_count[14])
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_stats_ready(b, "lamehip_batch_bitrate_hist", s);
    if (rc)
        return rc;
    for (int i = 0; i < 14; i++)
        bitrate_count[i] = b->h_st[(size_t) s].mode[i + 1][4];
    return 0;
}

extern "C" int
lamehip_batch_stereo_mode_hist(lamehip_batch * b, int s, int stmode_count[4])
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_stats_ready(b, "lamehip_batch_stereo_mode_hist", s);
    if (rc)
        return rc;
    for (int i = 0; i < 4; i++)
        stmode_count[i] = b->h_st[(size_t) s].mode[15][i];
    return 0;
}

extern "C" int
lamehip_batch_bitrate_stereo_mode_hist(lamehip_batch * b, int s, int bitrate_stmode_count[14][4])
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_stats_ready(b, "lamehip_batch_bitrate_stereo_mode_hist", s);
    if (rc)
        return rc;
    for (int j = 0; j < 14; j++)
        for (int i = 0; i < 4; i++)
            bitrate_stmode_count[j][i] = b->h_st[(size_t) s].mode[j + 1][i];
    return 0;
}

extern "C" int
lamehip_batch_block_type_hist(lamehip_batch * b, int s, int btype_count[6])
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_stats_ready(b, "lamehip_batch_block_type_hist", s);
    if (rc)
        return rc;
    for (int i = 0; i < 6; i++)
        btype_count[i] = b->h_st[(size_t) s].block[15][i];
    return 0;
}

extern "C" int
lamehip_batch_bitrate_block_type_hist(lamehip_batch * b, int s, int bitrate_btype_count[14][6])
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_stats_ready(b, "lamehip_batch_bitrate_block_type_hist", s);
    if (rc)
        return rc;
    for (int j = 0; j < 14; j++)
        for (int i = 0; i < 6; i++)
            bitrate_btype_count[j][i] = b->h_st[(size_t) s].block[j + 1][i];
    return 0;
}

/* the bit rates the rows 1..14 stand for (lame_bitrate_kbps) */
extern "C" int
lamehip_batch_bitrate_kbps(lamehip_batch * b, int bitrate_kbps[14])
{
    if (!b)
        return -1;
    if (!b->st_on) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_bitrate_kbps: the batch keeps no statistics (lamehip_batch_set_statistics)");
        return -1;
    }
    for (int i = 0; i < 14; i++)
        bitrate_kbps[i] = lh_tag_kbps(b->cfg.version, i + 1);
    return 0;
}

/* bytes of stream s produced since the last drain; -1 (and nothing taken) when they do not fit */
extern "C" int
lamehip_batch_drain(lamehip_batch * b, int s, unsigned char *out, int cap)
{
    int     n;
    if (!b || !b->incremental || s < 0 || s >= b->B)
        return -1;
    if (b->inc_pack) {
        /* the device packer: out of the round's pinned buffer */
        LhDrainRow & row = b->h_dr_rows.get()[s];
        if (!b->dr_have || row.n <= 0)
            return 0;
        if (!out || (long long) cap < row.n)
            return -1;
        n = (int) row.n;
        memcpy(out, b->h_round.get() + row.off, (size_t) n);
        b->dr_drained[(size_t) s] += n;
        row.n = 0;
        return n;
    }
    n = (int) b->pending[(size_t) s].size();
    if (n == 0)
        return 0;
    if (!out || cap < n)
        return -1;
    memcpy(out, b->pending[(size_t) s].data(), (size_t) n);
    b->pending[(size_t) s].clear();
    return n;
}

/* the same bytes in place: in the round's pinned buffer on the device packer, in a buffer of the batch's on the host
 * packer; valid until the next lamehip_batch_encode_available, _finish, _reset (host packer: or _drain_ptr of the stream).
 * Counts as a drain. */
extern "C" long
lamehip_batch_drain_ptr(lamehip_batch * b, int s, const unsigned char **bytes)
{
    if (!b || !b->incremental || s < 0 || s >= b->B || !bytes)
        return -1;
    *bytes = nullptr;
    if (b->inc_pack) {
        LhDrainRow & row = b->h_dr_rows.get()[s];
        if (!b->dr_have || row.n <= 0)
            return 0;
        long const n = (long) row.n;
        *bytes = b->h_round.get() + row.off;
        b->dr_drained[(size_t) s] += n;
        row.n = 0;
        return n;
    }
    b->handed[(size_t) s].clear();
    b->handed[(size_t) s].swap(b->pending[(size_t) s]);
    *bytes = b->handed[(size_t) s].empty() ? nullptr : b->handed[(size_t) s].data();
    return (long) b->handed[(size_t) s].size();
}

/* HIP-event time of the drain kernels (lh_drain.hip) of the last lamehip_batch_encode_available / _finish of a batch that
 * packs round by round on the device; 0 when none ran.  Not part of lamehip_batch_last_kernel_ms. */
extern "C" float
lamehip_batch_last_drain_ms(lamehip_batch * b)
{
    return b ? b->dr_ms : 0.0f;
}

extern "C" int
lamehip_batch_frames(lamehip_batch * b, int s)
{
    if (!b || s < 0 || s >= b->B)
        return -1;
    return b->nframes[(size_t) s];
}

extern "C" int
lamehip_batch_reset(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->incremental) {
        /* an incremental batch starts over: nothing fed, nothing staged, fresh packers, nothing left to drain */
        for (int s = 0; s < b->B; s++) {
            lh_bs_free(&b->packer[(size_t) s]);
            if (lh_bs_init_sized(&b->packer[(size_t) s], 65536) != 0)
                return -2;
            b->pending[(size_t) s].clear();
            b->handed[(size_t) s].clear();
        }
        b->fed.assign((size_t) b->B, 0);
        b->done.assign((size_t) b->B, 0);
        b->staged.assign((size_t) b->B, 0);
        b->have_last.assign((size_t) b->B, 0);
        b->stage_used = 0;
        b->stage_nseg = 0;
        b->ap_nseg = 0;
        b->ap_max_n = 0;
        b->finished = 0;
        /* (every slot holds a live stream again; what follows puts all records in HBM back, restarted slots' included) */
        batch_slots_open(b);
        /* (a batch that packs on the device: nothing handed out, the header walks at the slices' first bytes) */
        if (b->inc_pack && batch_drain_begin(b) != 0)
            return LAMEHIP_ERR_DEVICE;
        /* (a batch that converts round by round: every stream's converter back in front of its first sample) */
        for (LhRsCursor & c:b->rs_cur)
            lh_rs_cursor_init(&c);
        b->rs_conv.assign(b->rs_conv.size(), 0);
        b->h_tiles.clear();
        /* (... that measures ReplayGain round by round: every stream's analysis likewise, the carry in HBM included) */
        if (batch_gain_restart(b) != 0)
            return LAMEHIP_ERR_DEVICE;
    }
    /* (every stream back at the batch's own input rate; the classes made stay) */
    b->rs_scls.assign(b->rs_scls.size(), 0);
    /* every gain is forgotten, and every stream with it: the next encode measures all of them again */
    b->rg_measured = 0;
    b->rg_pending = 0;
    b->rg_ran = 0;
    b->rg_ms = 0;
    for (std::vector < double >&w:b->rg_win)
        w.clear();
    b->rg_dirty.assign((size_t) b->B, 1);
    /* (and every count) */
    if (batch_stats_zero(b, -1) != 0)
        return LAMEHIP_ERR_DEVICE;
    b->st_ran = b->st_timed = 0;
    b->st_ms = 0;
    return batch_reset_states(b);
}

/* The streams declared since their last conversion go through the device converter, on the batch's stream: the plan
 * travels first (the trunk only as far as it has grown since the last time), then one launch. */
static int
batch_convert_launch(lamehip_batch * b)
{
    int     max_blocks = 0;
    b->rs_ran = 0;
    b->h_tails.clear();
    b->h_rs_streams.clear();
    for (int s = 0; s < b->B; s++) {
        if (!b->rs_dirty[(size_t) s])
            continue;
        LhRsStream d;
        d.n = b->len_in[(size_t) s];
        d.stream = s;
        d.ntrunk = b->trunk.after[d.n / b->trunk.fs].nblk;
        d.tail_at = (int) b->h_tails.size();
        d.ntail = (int) b->tail[(size_t) s].size();
        b->h_tails.insert(b->h_tails.end(), b->tail[(size_t) s].begin(), b->tail[(size_t) s].end());
        b->h_rs_streams.push_back(d);
        if (d.ntrunk + d.ntail > max_blocks)
            max_blocks = d.ntrunk + d.ntail;
    }
    if (b->h_rs_streams.empty())
        return 0;
    long const ntrunk = b->trunk.after[b->trunk.nchunks].nblk;
    /* (twice what is needed; drained first: a conversion of the previous round may still be reading the old buffer) */
    bool    fresh = false;
    HIPCHK(b->d_rs_trunk.reserve((size_t) ntrunk, (size_t) ntrunk, b->stream, &fresh));
    if (fresh)
        b->rs_trunk_up = 0;
    if (ntrunk > b->rs_trunk_up) {
        HIPCHK(hipMemcpyAsync(b->d_rs_trunk.get() + b->rs_trunk_up, b->trunk.blk + b->rs_trunk_up,
                              (size_t) (ntrunk - b->rs_trunk_up) * sizeof(LhRsBlock), hipMemcpyHostToDevice, b->stream));
        b->rs_trunk_up = ntrunk;
    }
    HIPCHK(b->d_rs_tails.reserve(b->h_tails.size(), b->h_tails.size() + 64, b->stream));
    if (!b->h_tails.empty())
        HIPCHK(hipMemcpyAsync(b->d_rs_tails.get(), b->h_tails.data(), b->h_tails.size() * sizeof(LhRsBlock), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_rs_streams.get(), b->h_rs_streams.data(), b->h_rs_streams.size() * sizeof(LhRsStream), hipMemcpyHostToDevice,
                          b->stream));
    LhRsParams p;
    memset(&p, 0, sizeof(p));
    p.ratio = b->rs->ratio;
    p.m = b->stype != LH_PCM_S16 ? lh_pcm_matrix(b->stype, b->cfg.pcm_scale, b->cfg.pcm_mix, b->cfg.pcm_scale_r)
        : lh_rs_matrix(b->cfg.pcm_scale, b->cfg.pcm_mix, b->cfg.pcm_scale_r);
    p.taps = b->rs->taps;
    p.phases = b->rs->phases;
    p.channels = b->cfg.channels;
    p.one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    p.cap_in = b->cap;
    p.cap_out = b->capf;
    HIPCHK(hipEventRecord(b->ev_rs[0], b->stream));
    /* (a typed pool goes through the same kernel, its staging load in the pool's type: no ingest pass in between) */
    int const rc = b->stype != LH_PCM_S16
        ? lh_launch_resample_typed(b->stype, &p, b->d_rs_bank.get(), b->d_rs_trunk.get(), b->d_rs_tails.get(), b->d_rs_streams.get(),
                                   (int) b->h_rs_streams.size(), max_blocks, b->d_pcm.get(), b->d_pcmf.get(), (void *) (hipStream_t) b->stream)
        : lh_launch_resample(&p, b->d_rs_bank.get(), b->d_rs_trunk.get(), b->d_rs_tails.get(), b->d_rs_streams.get(), (int) b->h_rs_streams.size(),
                             max_blocks, b->d_pcm.get(), b->d_pcmf.get(), (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("conversion launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_rs[1], b->stream));
    b->rs_ran = 1;
    b->rs_dirty.assign((size_t) b->B, 0);
    return 0;
}

/* A typed batch that does not convert the rate: the streams declared since their last ingest go from the input pool into
 * the float pool (lh_ingest.hip), on the batch's stream; the list travels first, then one launch. */
static int
batch_ingest_launch(lamehip_batch * b)
{
    long long max_n = 0;
    b->in_ran = 0;
    b->h_in_streams.clear();
    for (int s = 0; s < b->B; s++) {
        if (!b->in_dirty[(size_t) s] || b->len[(size_t) s] <= 0)
            continue;
        LhInStream d;
        d.n = b->len[(size_t) s];
        d.stream = s;
        d.pad_ = 0;
        b->h_in_streams.push_back(d);
        if (d.n > max_n)
            max_n = d.n;
    }
    b->in_dirty.assign((size_t) b->B, 0);
    if (b->h_in_streams.empty())
        return 0;
    HIPCHK(hipMemcpyAsync(b->d_in_streams.get(), b->h_in_streams.data(), b->h_in_streams.size() * sizeof(LhInStream), hipMemcpyHostToDevice,
                          b->stream));
    LhInParams p;
    memset(&p, 0, sizeof(p));
    p.m = lh_pcm_matrix(b->stype, b->cfg.pcm_scale, b->cfg.pcm_mix, b->cfg.pcm_scale_r);
    p.channels = b->cfg.channels;
    p.one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    p.cap = b->cap;
    HIPCHK(hipEventRecord(b->ev_in[0], b->stream));
    int const rc = lh_launch_ingest(b->stype, &p, b->d_in_streams.get(), (int) b->h_in_streams.size(), max_n, b->d_pcm.get(), b->d_pcmf.get(),
                                    (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("ingest launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_in[1], b->stream));
    b->in_ran = 1;
    return 0;
}

/* ---- ReplayGain of a batch: the radio gain of every stream, measured by lh_gain.hip inside lamehip_batch_encode ---- */

static long
batch_gain_window(const lamehip_batch * b)
{
    return (b->cfg.samplerate * 1L + 20L - 1) / 20L;    /* 50 ms at the output rate, rounded up (lh_rg_start) */
}

/* the last launch's window sums come home: per stream the pairs, and the gain lh_replaygain.c makes of them */
static int
batch_gain_fetch(lamehip_batch * b)
{
    long const W = batch_gain_window(b);
    long long wins = 0;
    if (!b->rg_pending)
        return 0;
    for (const LhGainStream & d:b->h_rg_streams)
        wins += d.total / W;
    std::vector < double >all((size_t) (2 * wins));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (wins > 0)
        HIPCHK(hipMemcpy(all.data(), b->d_rg_pairs.get(), all.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (const LhGainStream & d:b->h_rg_streams) {
        long const nw = d.total / W;
        std::vector < double >&w = b->rg_win[(size_t) d.stream];
        w.assign(all.begin() + 2 * d.win_at, all.begin() + 2 * (d.win_at + nw));
        b->rg_tenths[(size_t) d.stream] = lh_gain_from_windows(w.data(), nw, W);
    }
    b->rg_pending = 0;
    return 0;
}

/* what a launch over h_rg_streams needs besides its streams */
static int
batch_gain_params(const lamehip_batch * b, LhGainParams * p)
{
    LhReplayGain probe;         /* (only for the row of the filter tables) */
    memset(p, 0, sizeof(*p));
    if (lh_rg_start(&probe, b->cfg.samplerate) != 0)
        return -1;
    memcpy(p->ky, lh_rg_yule[probe.rate_index], sizeof(p->ky));
    memcpy(p->kb, lh_rg_butter[probe.rate_index], sizeof(p->kb));
    p->m = lh_rs_matrix(b->cfg.pcm_scale, b->cfg.pcm_mix, b->cfg.pcm_scale_r);
    p->cap = batch_reads_floats(b) ? b->capf : b->cap;
    p->window = (int) batch_gain_window(b);
    p->fs = fs_of(b->cfg);
    p->channels = b->cfg.channels;
    p->one_plane = (b->cfg.channels == 1 && b->cfg.pcm_mix == 0.0f);
    {
        /* the mapping of the first filter's feedback, by the size of the launch (LH_GN_TAPS_BELOW: the faster one either side);
         * LAMEHIP_GAIN_LANES=0 / 1 (measurement aid, tools/replaygain_bench.py) forces the taps across the lanes of a row / the
         * feedback in lanes 0 and 1 -- the same sums either way, so a batch measured round by round may change it every round */
        const char *e = getenv("LAMEHIP_GAIN_LANES");
        p->taps = e ? atoi(e) != 1 : (int) b->h_rg_streams.size() < LH_GN_TAPS_BELOW;
    }
    return 0;
}

/* The streams declared since their last analysis go through the gain kernel, on the batch's stream: the host plans --
 * which blocks the handle API would have handed to lh_rg_block, from the lengths alone --, the plan travels, one launch. */
static int
batch_gain_launch(lamehip_batch * b)
{
    int const fs = fs_of(b->cfg), mfn = mfn_of(b->cfg);
    long const W = batch_gain_window(b);
    long long wins = 0;
    int     max_trunk = 0;
    LhResampler *host_rs = nullptr;
    /* (the pairs of the launch before this one share the buffer) */
    if (batch_gain_fetch(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    b->h_rg_streams.clear();
    b->h_rg_tails.clear();
    for (int s = 0; s < b->B; s++) {
        if (!b->rg_dirty[(size_t) s])
            continue;
        LhGainStream d;
        long    total = 0;
        memset(&d, 0, sizeof(d));
        d.n = b->len[(size_t) s];
        d.stream = s;
        d.win_at = wins;
        d.tail_at = (int) b->h_rg_tails.size();
        if (b->dev_rs) {
            /* the made counts of the stream's conversion plan: the trunk all streams share, then its own tail */
            d.ntrunk = b->trunk.after[b->len_in[(size_t) s] / b->trunk.fs].nblk;
            for (const LhRsBlock & k:b->tail[(size_t) s])
                b->h_rg_tails.push_back(k.made);
            total = b->len[(size_t) s];
        }
        else {
            /* no conversion: whole frames' worth from position 0 (not listed), the remainder, the flush's zeros; a batch that
             * converts on the host: the plan of the conversion it made in lamehip_batch_set_pcm, listed whole */
            long const n_in = b->rate_in ? b->rg_len_in[(size_t) s] : b->len[(size_t) s];
            if (b->rate_in && !host_rs) {
                host_rs = (LhResampler *) malloc(sizeof(LhResampler));
                if (!host_rs) {
                    snprintf(g_err, sizeof(g_err), "out of memory (gain plan)");
                    return -2;
                }
                lh_rs_init(host_rs, b->rate_in, b->cfg.samplerate);
            }
            std::vector < int >blocks(64);
            /* (a stream of a converting batch that was never handed over has no converted signal, not even a flush's) */
            bool const none = b->rate_in && b->len[(size_t) s] == 0;
            int     nb = none ? 0 : lh_gain_plan(host_rs, fs, mfn, n_in, blocks.data(), (int) blocks.size(), &total);
            if (nb > (int) blocks.size()) {
                blocks.resize((size_t) nb);
                nb = lh_gain_plan(host_rs, fs, mfn, n_in, blocks.data(), (int) blocks.size(), &total);
            }
            if (nb < 0 || (b->rate_in && total != b->len[(size_t) s])) {
                free(host_rs);
                snprintf(g_err, sizeof(g_err), "gain plan: stream %d's blocks do not add up to its length", s);
                return -1;
            }
            d.ntrunk = b->rate_in ? 0 : (int) (n_in / fs);
            b->h_rg_tails.insert(b->h_rg_tails.end(), blocks.begin() + d.ntrunk, blocks.begin() + nb);
        }
        if (total > LH_GN_MAX_TOTAL) {
            free(host_rs);
            snprintf(g_err, sizeof(g_err), "lamehip_batch_encode: stream %d is too long for the ReplayGain analysis (%ld samples)", s, total);
            return -1;
        }
        d.total = (int) total;
        d.ntail = (int) b->h_rg_tails.size() - d.tail_at;
        if (b->dev_rs && d.ntrunk > max_trunk)
            max_trunk = d.ntrunk;
        wins += total / W;
        b->h_rg_streams.push_back(d);
    }
    free(host_rs);
    if (b->h_rg_streams.empty()) {
        b->rg_measured = 1;     /* (nothing declared since the last analysis: every result stands) */
        return 0;
    }
    b->h_rg_trunk.resize((size_t) max_trunk);
    for (int j = 0; j < max_trunk; j++)
        b->h_rg_trunk[(size_t) j] = b->trunk.blk[j].made;
    /* (drained first: the analysis of the previous round may still be reading the old buffers) */
    HIPCHK(b->d_rg_tails.reserve(b->h_rg_tails.size() + 1, 64, b->stream));
    HIPCHK(b->d_rg_trunk.reserve(b->h_rg_trunk.size() + 1, b->h_rg_trunk.size(), b->stream));
    HIPCHK(b->d_rg_pairs.reserve((size_t) (2 * wins + 2), (size_t) (wins / 4), b->stream));
    if (!b->h_rg_tails.empty())
        HIPCHK(hipMemcpyAsync(b->d_rg_tails.get(), b->h_rg_tails.data(), b->h_rg_tails.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
    if (!b->h_rg_trunk.empty())
        HIPCHK(hipMemcpyAsync(b->d_rg_trunk.get(), b->h_rg_trunk.data(), b->h_rg_trunk.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_rg_streams.get(), b->h_rg_streams.data(), b->h_rg_streams.size() * sizeof(LhGainStream), hipMemcpyHostToDevice,
                          b->stream));
    LhGainParams p;
    if (batch_gain_params(b, &p) != 0)
        return -1;
    HIPCHK(hipEventRecord(b->ev_rg[0], b->stream));
    int const rc = lh_launch_gain(batch_reads_floats(b), &p, b->d_rg_streams.get(), (int) b->h_rg_streams.size(),
                                  b->dev_rs ? b->d_rg_trunk.get() : nullptr, b->d_rg_tails.get(),
                                  batch_reads_floats(b) ? (const void *) b->d_pcmf.get() : (const void *) b->d_pcm.get(), b->d_rg_pairs.get(),
                                  (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("gain launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_rg[1], b->stream));
    /* queued: only now do the streams count as analysed (a failure above leaves them declared, and the getters refusing) */
    b->rg_dirty.assign((size_t) b->B, 0);
    b->rg_measured = 1;
    b->rg_ran = 1;
    b->rg_pending = 1;
    return 0;
}

/* A round of a batch that measures ReplayGain round by round (lamehip_batch_encode_available / _finish): the streams with
 * blocks planned since the last round go through lh_gain_resume_kernel, ONE launch on the batch's stream between ev_rg[0] and
 * ev_rg[1], behind the append and conversion launches -- every sample the blocks cover is in the pool the kernels read,
 * counted in fed[] (in rs_cur[].fed where the batch converts), and what lies beyond is generated zeros, the flush's --;
 * the round's window sums follow the launch home.  A stream without blocks is not part of the launch: its carry stays. */
static int
batch_gain_round(lamehip_batch * b)
{
    long const W = batch_gain_window(b);
    long long wins = 0;
    b->rg_ran = 0;
    b->h_rg_streams.clear();
    b->h_rg_tails.clear();
    for (int s = 0; s < b->B; s++) {
        std::vector < int >const &g = b->rg_blk[(size_t) s];
        if (g.empty())
            continue;
        LhGainStream d;
        long long const heard = b->rg_heard[(size_t) s];
        long long total = 0;
        for (int k:g)
            total += k;
        memset(&d, 0, sizeof(d));
        d.n = b->inc_rs ? b->rs_cur[(size_t) s].fed : (long long) b->fed[(size_t) s];
        d.win_at = wins;
        d.total = (int) total;
        d.stream = s;
        d.tail_at = (int) b->h_rg_tails.size();
        d.ntail = (int) g.size();
        b->h_rg_tails.insert(b->h_rg_tails.end(), g.begin(), g.end());
        wins += (heard + total) / W - heard / W;
        b->h_rg_streams.push_back(d);
    }
    if (b->h_rg_streams.empty())
        return 0;
    /* (nothing of an earlier round is in flight: a round ends with a wait) */
    HIPCHK(b->d_rg_tails.reserve(b->h_rg_tails.size() + 1, b->h_rg_tails.size(), b->stream));
    HIPCHK(b->d_rg_pairs.reserve((size_t) (2 * wins + 2), (size_t) (2 * wins), b->stream));
    b->h_rg_round.resize((size_t) (2 * wins));
    HIPCHK(hipMemcpyAsync(b->d_rg_tails.get(), b->h_rg_tails.data(), b->h_rg_tails.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_rg_streams.get(), b->h_rg_streams.data(), b->h_rg_streams.size() * sizeof(LhGainStream), hipMemcpyHostToDevice,
                          b->stream));
    LhGainParams p;
    if (batch_gain_params(b, &p) != 0)
        return -1;
    HIPCHK(hipEventRecord(b->ev_rg[0], b->stream));
    int const rc = lh_launch_gain_resume(batch_reads_floats(b), &p, b->d_rg_streams.get(), (int) b->h_rg_streams.size(), b->d_rg_tails.get(),
                                         batch_reads_floats(b) ? (const void *) b->d_pcmf.get() : (const void *) b->d_pcm.get(),
                                         b->d_rg_pairs.get(), b->d_rg_carry.get(), (void *) (hipStream_t) b->stream);
    if (rc)
        return set_err("gain launch", (hipError_t) rc);
    HIPCHK(hipEventRecord(b->ev_rg[1], b->stream));
    if (wins > 0)
        HIPCHK(hipMemcpyAsync(b->h_rg_round.data(), b->d_rg_pairs.get(), b->h_rg_round.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    b->rg_ran = 1;
    return 0;
}

/* behind the round's wait: the launch's time (lamehip_batch_last_gain_ms), every stream's new windows join its list, the
 * blocks are done with; the streams the round ends: the flush was part of the round, the gains are made of the windows
 * (lh_replaygain.c); end: that was the last round of all */
static void
batch_gain_round_done(lamehip_batch * b, int end)
{
    long const W = batch_gain_window(b);
    if (!b->inc_rg)
        return;
    b->rg_ms = 0;
    if (b->rg_ran) {
        if (hipEventElapsedTime(&b->rg_ms, b->ev_rg[0], b->ev_rg[1]) != hipSuccess) {
            (void) hipGetLastError();
            b->rg_ms = 0;
        }
        for (const LhGainStream & d:b->h_rg_streams) {
            long long &heard = b->rg_heard[(size_t) d.stream];
            long long const nw = (heard + d.total) / W - heard / W;
            std::vector < double >&w = b->rg_win[(size_t) d.stream];
            w.insert(w.end(), b->h_rg_round.begin() + 2 * d.win_at, b->h_rg_round.begin() + 2 * (d.win_at + nw));
            heard += d.total;
            b->rg_blk[(size_t) d.stream].clear();
        }
        b->h_rg_streams.clear();
    }
    /* (the streams the round flushed: their gains are final) */
    for (int s = 0; s < b->B; s++)
        if (b->ending[(size_t) s]) {
            b->rg_tenths[(size_t) s] = lh_gain_from_windows(b->rg_win[(size_t) s].data(), (long) (b->rg_win[(size_t) s].size() / 2), W);
            b->rg_final[(size_t) s] = 1;
        }
    if (end)
        b->rg_closed = 1;
}

/* the tag of stream s carries its gain when the batch measures it */
static int
batch_tag_gain(lamehip_batch * b, int s, LhVbrTag * v)
{
    LhDeviceScope const on_device(b->device);
    if (!b->rg_on || !b->rg_measured)
        return 0;
    if (batch_gain_fetch(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    v->radio_gain_on = 1;
    v->radio_gain = b->rg_tenths[(size_t) s];
    return 0;
}

/* ReplayGain for every stream of the batch: lamehip_batch_encode measures the radio gain the handle API would report for
 * the same samples fed a frame's worth per lame_encode_buffer call (lame_set_findReplayGain), and the tagged outputs
 * carry it.  Before lamehip_batch_encode; not for incremental batches.  The proto's own setting is not inherited. */
extern "C" int
lamehip_batch_set_replaygain(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_replaygain: this batch is fed with lamehip_batch_append (incremental use)");
        return -1;
    }
    if (!on || b->rg_on) {
        b->rg_on = on != 0 && b->rg_on;
        b->inc_rg = b->inc_rg && b->rg_on;      /* (round by round is this analysis' too) */
        return 0;
    }
    /* everything new first: a failure leaves the batch as it was */
    LhDevBuf < LhGainStream > streams;
    LhEvent ev[2];
    hipError_t e = streams.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = ev[0].create();
    if (e == hipSuccess)
        e = ev[1].create();
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_replaygain: device allocation", e);
    }
    b->d_rg_streams = std::move(streams);
    b->ev_rg[0] = std::move(ev[0]);
    b->ev_rg[1] = std::move(ev[1]);
    b->rg_win.assign((size_t) b->B, std::vector < double >());
    b->rg_tenths.assign((size_t) b->B, 0);
    b->rg_dirty.assign((size_t) b->B, 1);       /* whatever has been declared so far is measured by the next encode */
    b->rg_measured = 0;
    b->rg_pending = 0;
    b->rg_on = 1;
    return 0;
}

/* ReplayGain round by round, for an incremental batch: once lamehip_batch_append (or one of its siblings) feeds the batch,
 * every append is a call of the reference entry point the batch's sample type is named after, made with
 * lame_set_findReplayGain(1); every lamehip_batch_encode_available and lamehip_batch_finish analyses what was appended since
 * the last round -- lamehip_batch_finish the flush as well --, lamehip_batch_get_gain_windows returns the windows finished so
 * far after any round, and lamehip_batch_radio_gain, after lamehip_batch_finish, what lame_get_RadioGain returns on a handle
 * fed the same calls.  Until the first append the batch measures whole streams, as after lamehip_batch_set_replaygain(b, 1).
 * Only before any PCM is handed over; a batch that converts the rate needs lamehip_batch_set_incremental_resampling first;
 * not for a batch that packs on the device.  on = 0 puts the batch back as it was. */
extern "C" int
lamehip_batch_set_incremental_replaygain(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->pcm_given || b->encoded || b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_replaygain: only before any PCM is handed over");
        return -1;
    }
    if (!on || b->inc_rg) {
        if (!on && b->inc_rg) {
            b->inc_rg = 0;
            b->rg_on = b->rg_was_on;
        }
        return 0;
    }
    if (b->dev_pack && !b->inc_pack) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_replaygain: not for a batch that packs on the device "
                 "(lamehip_batch_set_device_packing), which incremental use does not unless lamehip_batch_set_incremental_packing "
                 "was called first");
        return -1;
    }
    if (b->rate_in && !b->inc_rs) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_replaygain: this batch converts the sample rate, "
                 "lamehip_batch_set_incremental_resampling first (the analysis follows the conversion's calls)");
        return -1;
    }
    /* everything new first: a failure leaves the batch as it was */
    int const was_on = b->rg_on;
    LhDevBuf < LhGainCarry > carry;
    std::vector < LhGainCursor > cur;
    std::vector < std::vector < int > >blk;
    std::vector < long long >heard;
    hipError_t e = carry.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = hipMemset(carry.get(), 0, (size_t) b->B * sizeof(LhGainCarry));
    try {
        LhGainCursor first;
        lh_gain_cursor_init(&first);
        cur.assign((size_t) b->B, first);
        blk.assign((size_t) b->B, std::vector < int >());
        heard.assign((size_t) b->B, 0);
    }
    catch(const std::bad_alloc &) {
        e = hipErrorOutOfMemory;
    }
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_incremental_replaygain: allocation", e);
    }
    if (!was_on) {
        int const rc = lamehip_batch_set_replaygain(b, 1);      /* (the launch's records, the events, the lists of windows) */
        if (rc != 0)
            return rc;
    }
    b->d_rg_carry = std::move(carry);
    b->rg_cur = std::move(cur);
    b->rg_blk = std::move(blk);
    b->rg_heard = std::move(heard);
    b->rg_was_on = was_on;
    b->rg_closed = 0;
    b->inc_rg_max = LH_GN_MAX_TOTAL;
    {
        /* LAMEHIP_INC_RG_MAX=n, looked at here: the appends count the analysis as taking n samples per stream, no more than it
         * does (test aid: the real limit is beyond any pool a test would allocate) */
        const char *m = getenv("LAMEHIP_INC_RG_MAX");
        long long const v = m ? strtoll(m, nullptr, 10) : 0;
        if (v > 0 && v < b->inc_rg_max)
            b->inc_rg_max = v;
    }
    b->inc_rg = 1;
    return 0;
}

/* who: one of the getters; final: it needs the gain, which an incremental batch has after lamehip_batch_finish */
static int
batch_gain_ready(lamehip_batch * b, int s, const char *who, bool final = false)
{
    if (!b || s < 0 || s >= b->B)
        return -1;
    if (b->inc_rg && b->incremental) {
        /* (or after the round that ended the stream alone: lamehip_batch_end_stream) */
        if (final && !b->rg_final[(size_t) s]) {
            snprintf(g_err, sizeof(g_err), "%s: an incremental batch's gain exists after lamehip_batch_finish (as lame_get_RadioGain's after "
                     "lame_encode_flush)", who);
            return -1;
        }
        return 0;               /* (the windows came home with the round) */
    }
    if (!b->rg_on || !b->rg_measured) {
        snprintf(g_err, sizeof(g_err), "%s: no lamehip_batch_encode with lamehip_batch_set_replaygain on has run", who);
        return -1;
    }
    return batch_gain_fetch(b) != 0 ? LAMEHIP_ERR_DEVICE : 0;
}

/* stream s's radio gain in tenths of a dB as the LAME tag stores it (lame_get_RadioGain); 0 when the stream has no
 * finished window.  Waits for the batch's stream. */
extern "C" int
lamehip_batch_radio_gain(lamehip_batch * b, int s, int *tenths_db)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = tenths_db ? batch_gain_ready(b, s, "lamehip_batch_radio_gain", true) : -1;
    if (rc)
        return rc;
    *tenths_db = b->rg_tenths[(size_t) s];
    return 0;
}

/* test accessor: the window sums the kernel left for stream s, (lsum, rsum) per finished 50 ms window; writes the first
 * cap_windows pairs and returns the number of windows, or a negative code */
extern "C" long
lamehip_batch_get_gain_windows(lamehip_batch * b, int s, double *lr_pairs, long cap_windows)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int const rc = batch_gain_ready(b, s, "lamehip_batch_get_gain_windows");
    if (rc)
        return rc;
    std::vector < double >const &w = b->rg_win[(size_t) s];
    long const nw = (long) (w.size() / 2), k = nw < cap_windows ? nw : cap_windows;
    if (k > 0 && lr_pairs)
        memcpy(lr_pairs, w.data(), (size_t) k * 2 * sizeof(double));
    return nw;
}

/* HIP-event time of the gain kernel of the last lamehip_batch_encode (after lamehip_batch_sync); 0 when none ran.  Not part
 * of lamehip_batch_last_kernel_ms. */
extern "C" float
lamehip_batch_last_gain_ms(lamehip_batch * b)
{
    return b ? b->rg_ms : 0.0f;
}

/* The byte pool's slice of stream s (device packing; else 0): room for every frame at the largest frame size the settings
 * allow, +1 for CBR padding.  lamehip_batch_encode lays the streams out with it, lamehip_batch_reserve sizes the pool by it. */
static int
batch_frame_max(const lamehip_batch * b)
{
    int const top = (b->cfg.vbr == 0) ? b->cfg.bitrate_index : b->cfg.vbr_max_bitrate_index;
    /* (the row of the stream's MPEG version: an MPEG-2 / 2.5 index stands for half the MPEG-1 rate or less) */
    return (b->cfg.version + 1) * 72000 * lh_tag_kbps(b->cfg.version, top & 15) / b->cfg.samplerate + 1;
}

static long long
batch_stream_bytes(const lamehip_batch * b, int s)
{
    return b->dev_pack ? (long long) b->nframes[(size_t) s] * batch_frame_max(b) : 0;
}

/* device tagging: the room in front of every stream's audio in the byte pool -- the tag frame's size, constant per batch; 0
 * with the switch off, or when the tag does not fit a frame (lh_tag_init) */
static int
batch_tag_room(const lamehip_batch * b)
{
    return (b->dev_pack && b->dev_tag) ? b->tag_p.total : 0;
}

/* room for a launch of `total' frames whose streams' slices add up to `bytes_total' */
static int
batch_pools_reserve(lamehip_batch * b, long long total, long long bytes_total)
{
    if (b->dev_pack)
        HIPCHK(b->d_bytes.reserve((size_t) bytes_total));
    HIPCHK(b->d_out.reserve((size_t) total));
    return 0;
}

extern "C" int
lamehip_batch_encode(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    long long total = 0, bytes_total = 0;
    if (!b)
        return -1;
    if (batch_refuse_own_rates(b, "lamehip_batch_encode"))
        return -1;
    if (b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_encode: this batch is fed with lamehip_batch_append (incremental use)");
        return -1;
    }
    /* a batch that has been encoded starts over: every call encodes the streams from their first
     * sample, so the carried state must be the initial one */
    if (b->encoded && batch_reset_states(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    int const room = batch_tag_room(b);
    for (int s = 0; s < b->B; s++) {
        LhStreamDesc & d = b->h_desc[(size_t) s];
        b->out_off[(size_t) s] = total;
        d.pcm_l = ((long long) s * 2) * (batch_reads_floats(b) ? b->capf : b->cap);
        d.pcm_r = ((long long) s * 2 + 1) * (batch_reads_floats(b) ? b->capf : b->cap);
        d.pcm_base = 0;
        d.nsamples = b->len[(size_t) s];
        d.out_index = total;
        d.frame_begin = 0;
        d.frame_end = b->nframes[(size_t) s];
        d.flush = 1;
        d.mid_rel = 0;
        d.bytes_base = bytes_total + room;      /* (device tagging: the tag frame's room comes first) */
        d.bytes_cap = batch_stream_bytes(b, s);
        b->bytes_off[(size_t) s] = d.bytes_base;
        bytes_total += room + d.bytes_cap;
        total += b->nframes[(size_t) s];
    }
    b->tagged = b->dev_pack && b->dev_tag;
    b->tag_room = room;
    b->tag_ran = 0;
    {
        int const rc = batch_pools_reserve(b, total, bytes_total);
        if (rc)
            return rc;
    }
    if (b->n_dirty && lamehip_batch_upload(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    if (b->up_pending) {
        HIPCHK(hipStreamWaitEvent(b->stream, b->ev_up, 0));
        b->up_pending = 0;
    }
    if (b->down_pending) {      /* the previous round's bytes must have left d_bytes */
        HIPCHK(hipStreamWaitEvent(b->stream, b->ev_down, 0));
        b->down_pending = 0;
    }
    HIPCHK(hipMemcpyAsync(b->d_desc.get(), b->h_desc.data(), (size_t) b->B * sizeof(LhStreamDesc),
                          hipMemcpyHostToDevice, b->stream));
    if (room > 0) {
        /* device tagging: what the tag kernel cannot know -- every stream's end padding -- travels with the descriptors */
        for (int s = 0; s < b->B; s++) {
            b->h_tag_pad[(size_t) s] = batch_padding(b, s);
            b->tag_patched[(size_t) s] = 0;
        }
        HIPCHK(hipMemcpyAsync(b->d_tag_pad.get(), b->h_tag_pad.data(), (size_t) b->B * sizeof(int), hipMemcpyHostToDevice, b->stream));
    }
    /* device conversion, or the ingest of a typed pool: behind the upload wait, in front of the analysis kernels */
    b->in_ran = 0;
    if (b->dev_rs) {
        int const rc = batch_convert_launch(b);
        if (rc)
            return rc;
    }
    else if (b->stype != LH_PCM_S16) {
        int const rc = batch_ingest_launch(b);
        if (rc)
            return rc;
    }
    /* ReplayGain: behind the conversion / ingest, in front of the analysis kernels, once per call whatever the windows */
    b->rg_ran = 0;
    if (b->rg_on) {
        int const rc = batch_gain_launch(b);
        if (rc)
            return rc;
    }
    /* statistics: every call counts the streams from their first frame */
    if (b->st_on && batch_stats_zero(b, -1) != 0)
        return LAMEHIP_ERR_DEVICE;
    /* (what the launch will be -- and the pool it needs -- before the device's launch order is taken: an allocation of tens
     * of GB must not keep other batches' launches waiting) */
    LhLaunchPlan plan;
    {
        int const rc = batch_plan(b, b->h_desc.data(), &plan);
        if (rc)
            return rc;
    }
    {
        /* Launches that fill the device run one after the other, in launch order, whatever HIP streams their batches
         * own: a launch of >= 512 streams keeps every SIMD's register file and every CU's LDS (2 x 256 VGPRs, 4 x 40 KB),
         * so a second one has nothing to gain from being dispatched early -- and measured on the MI355X it loses: dispatched
         * while the first still runs, its workgroups end up resident in two rounds (kernel 176 ms alone, 329 ms behind
         * another launch, every stream's own cycle count unchanged; tools/e2e_diag2.py), which cost the two-batch pipeline a
         * third of its rate.  Copies on the batches' copy streams overlap the kernels as before. */
        LhLaunchSerial & ser = launch_serial(b->device);
        std::lock_guard < std::mutex > hold(ser.lock);
        int const big = (b->B >= 512);
        if (big && ser.ev)
            HIPCHK(hipStreamWaitEvent(b->stream, ser.ev, 0));
        int     rc = batch_launch(b, batch_reads_floats(b) ? (const int16_t *) 0 : b->d_pcm.get(),
                                  batch_reads_floats(b) ? b->d_pcmf.get() : (const float *) 0,
                                  b->d_desc.get(), plan, b->dev_pack ? b->d_bytes.get() : (uint8_t *) 0);
        if (rc)
            return rc;
        if (b->dev_pack) {
            /* the two words per stream lamehip_batch_fetch copies first: gathered here, inside the serial order -- as a
             * launch of its own behind the NEXT batch's kernel it found no free register file until that kernel was over
             * (all of a launch's streams end within a frame or two of each other), and its batch came home one kernel late */
            if (batch_copy_streams(b) != 0)
                return LAMEHIP_ERR_DEVICE;
            HIPCHK(b->d_sum.reserve((size_t) b->B * 2));
            rc = lh_launch_summary(b->d_state.get(), b->d_sum.get(), b->B, (void *) (hipStream_t) b->stream);
            if (rc)
                return set_err("summary launch", (hipError_t) rc);
            if (room > 0) {
                /* device tagging: the tag frames, right behind -- in the serial order for the summary's reason, and in front
                 * of ev_sum, which the fetch's copy of the bytes waits for */
                HIPCHK(hipEventRecord(b->ev_tag[0], b->stream));
                rc = lh_launch_tag(&b->tag_p, b->d_desc.get(), b->d_state.get(), b->d_out.get(), b->d_bytes.get(), b->d_tag_tmpl.get(),
                                   b->d_tag_pad.get(), b->B, (void *) (hipStream_t) b->stream);
                if (rc)
                    return set_err("tag launch", (hipError_t) rc);
                HIPCHK(hipEventRecord(b->ev_tag[1], b->stream));
                b->tag_ran = 1;
            }
            HIPCHK(hipEventRecord(b->ev_sum, b->stream));
        }
        if (big) {
            if (!ser.ev)
                HIPCHK(hipEventCreateWithFlags(&ser.ev, hipEventDisableTiming));
            HIPCHK(hipEventRecord(ser.ev, b->stream));
        }
    }
    b->launched = 1;
    b->encoded = 1;
    b->fetched = 0;
    return 0;
}

/* Device-packed batches: start the way back -- per stream (bytes, status), then the bytes themselves, into
 * pinned host memory, asynchronously on the batch's stream (behind the kernel).  lamehip_batch_bytes_ptr /
 * lamehip_batch_get_bytes_all wait for it.  Calling it right after lamehip_batch_encode lets the copies of this
 * batch run under the next batch's kernel. */
extern "C" int
lamehip_batch_fetch(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    long long total = 0;
    if (!b || !b->encoded || !b->dev_pack)
        return -1;
    if (b->fetched)
        return 0;
    for (int s = 0; s < b->B; s++)
        total += b->tag_room + b->h_desc[(size_t) s].bytes_cap;
    HIPCHK(b->d_sum.reserve((size_t) b->B * 2));
    HIPCHK(b->h_sum.reserve((size_t) b->B * 2));
    HIPCHK(b->h_bytes.reserve((size_t) total));
    if (batch_copy_streams(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    /* (the summary words were gathered right behind the kernel: lamehip_batch_encode) */
    HIPCHK(hipStreamWaitEvent(b->down_stream, b->ev_sum, 0));
    HIPCHK(hipMemcpyAsync(b->h_sum.get(), b->d_sum.get(), (size_t) b->B * 2 * sizeof(long long), hipMemcpyDeviceToHost, b->down_stream));
    if (total > 0)
        HIPCHK(hipMemcpyAsync(b->h_bytes.get(), b->d_bytes.get(), (size_t) total, hipMemcpyDeviceToHost, b->down_stream));
    HIPCHK(hipEventRecord(b->ev_down, b->down_stream));
    b->down_pending = 1;
    b->fetched = 1;
    return 0;
}

/* stream s's finished bytes in the batch's pinned buffer (valid until the batch is encoded again): returns
 * their number, or a negative code */
extern "C" long
lamehip_batch_bytes_ptr(lamehip_batch * b, int s, const unsigned char **p)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    long    n;
    if (!b || s < 0 || s >= b->B || !b->encoded || !b->dev_pack || !p)
        return -1;
    if (!b->fetched && lamehip_batch_fetch(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    HIPCHK(hipStreamSynchronize(b->down_stream));
    if (b->h_sum.get()[2 * s + 1] != 0) {
        snprintf(g_err, sizeof(g_err), "device bit packer reported status %d for stream %d", (int) b->h_sum.get()[2 * s + 1], s);
        return LAMEHIP_ERR_PAYLOAD;
    }
    n = (b->nframes[(size_t) s] == 0) ? 0 : (long) b->h_sum.get()[2 * s];
    *p = b->h_bytes.get() + b->bytes_off[(size_t) s];
    return n;
}

/* Device bit packing: the kernel also assembles each stream's finished MP3 bytes in HBM
 * (lh_dev_emit.h); lamehip_batch_get_bytes then copies them out, no host packer involved.
 * Set before lamehip_batch_encode. */
extern "C" int
lamehip_batch_set_device_packing(lamehip_batch * b, int on)
{
    if (!b)
        return -1;
    if (b->inc_pack && b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_device_packing: this batch is fed with lamehip_batch_append and packs its rounds "
                 "on the device (lamehip_batch_set_incremental_packing)");
        return -1;
    }
    b->dev_pack = on != 0;
    if (!b->dev_pack) {
        b->dev_tag = 0;         /* (the tag frames go in front of the device packer's bytes) */
        b->inc_pack = 0;        /* (and the rounds of an incremental batch are the device packer's) */
        b->inc_tag = 0;         /* (and so are their tag frames) */
    }
    return 0;
}

/* Incremental use of a batch that packs on the device (lamehip_batch_set_device_packing first): the appends are accepted,
 * every lamehip_batch_encode_available / _finish runs the encode kernel with its bit packer on every stream's fixed slice of
 * the byte pool and, behind it, the drain kernels (lh_drain.hip), and lamehip_batch_drain / _drain_ptr hand out finished MP3
 * bytes that came home in one copy -- no LhFrameOut record crosses to the host and no host packer runs.  Only before any PCM
 * is handed over; not with device tagging (an incremental batch's tag frames are lamehip_batch_set_incremental_tagging's);
 * lamehip_batch_set_incremental_resampling, _replaygain and _tagging go on top when called after it.  on = 0 puts the batch back as it was. */
extern "C" int
lamehip_batch_set_incremental_packing(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (!b->dev_pack) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_packing: for a batch that packs on the device "
                 "(lamehip_batch_set_device_packing first)");
        return -1;
    }
    if (b->pcm_given || b->encoded || b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_packing: only before any PCM is handed over");
        return -1;
    }
    if (b->dev_tag) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_packing: not with lamehip_batch_set_device_tagging "
                 "(an incremental batch has no tagged output)");
        return -1;
    }
    if (!on || b->inc_pack) {
        if (!on && b->inc_pack && (b->inc_rs || b->inc_rg)) {
            snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_packing: lamehip_batch_set_incremental_resampling / _replaygain "
                     "were switched on on top of it; switch them off first");
            return -1;
        }
        if (!on && b->inc_pack && b->inc_tag) {
            snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_packing: lamehip_batch_set_incremental_tagging was switched on "
                     "on top of it; switch it off first");
            return -1;
        }
        b->inc_pack = on != 0 && b->inc_pack;
        return 0;
    }
    /* everything new first: a failure leaves the batch as it was */
    LhDevBuf < long long >drained, carry;
    LhDevBuf < LhDrainRow > rows;
    LhPinned < LhDrainRow > h_rows;
    LhEvent ev[2];
    std::vector < long long >h_drained;
    hipError_t e = drained.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = carry.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = rows.alloc((size_t) b->B + 1);
    if (e == hipSuccess)
        e = h_rows.alloc((size_t) b->B + 1);
    if (e == hipSuccess)
        e = ev[0].create();
    if (e == hipSuccess)
        e = ev[1].create();
    try {
        h_drained.assign((size_t) b->B, 0);
    }
    catch(const std::bad_alloc &) {
        e = hipErrorOutOfMemory;
    }
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_incremental_packing: allocation", e);
    }
    memset(h_rows.get(), 0, ((size_t) b->B + 1) * sizeof(LhDrainRow));
    b->d_dr_drained = std::move(drained);
    b->d_dr_carry = std::move(carry);
    b->d_dr_rows = std::move(rows);
    b->h_dr_rows = std::move(h_rows);
    b->ev_dr[0] = std::move(ev[0]);
    b->ev_dr[1] = std::move(ev[1]);
    b->dr_drained = std::move(h_drained);
    b->dr_have = 0;
    b->inc_pack = 1;
    return 0;
}

/* Device tagging, on top of device packing: behind the encode kernel one more kernel (lh_tag.hip) writes every stream's
 * final Xing/Info + LAME tag frame into HBM, directly in front of the stream's audio bytes, and lamehip_batch_fetch brings
 * complete file images home (lamehip_batch_image_ptr / _get_images_all; lamehip_batch_get_bytes_tagged copies the same
 * image instead of walking and summing the bytes on the host).  The audio getters return what they returned.  Before
 * lamehip_batch_encode; may be switched between launches.  When the tag does not fit a frame (lh_tag_init) the images are
 * the audio alone. */
extern "C" int
lamehip_batch_set_device_tagging(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_device_tagging: this batch is fed with lamehip_batch_append (incremental use), "
                 "which takes the host packer; the tag frames go in front of the device packer's bytes (lamehip_batch_set_device_packing)");
        return -1;
    }
    if (!b->dev_pack) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_device_tagging: for a batch that packs on the device "
                 "(lamehip_batch_set_device_packing first)");
        return -1;
    }
    if (on && b->inc_pack) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_device_tagging: this batch packs its rounds on the device "
                 "(lamehip_batch_set_incremental_packing), and an incremental batch has no tagged output");
        return -1;
    }
    if (!on || b->d_tag_pad.get()) {
        b->dev_tag = on != 0;
        return 0;
    }
    /* everything new first: a failure leaves the batch as it was */
    LhVbrTag v;
    LhTagParams p;
    int const total = lh_tag_init(&v, &b->cfg);
    if (b->rate_in)
        v.samplerate_in = b->rate_in;
    lh_tag_params(&v, &b->cfg, &p);
    LhDevBuf < unsigned char >tmpl;
    LhDevBuf < int >pad;
    LhEvent ev[2];
    std::vector < int >h_pad;
    std::vector < char >patched;
    std::vector < unsigned char >h_tmpl((size_t) (total > 0 ? total : 1), 0);
    if (total > 0)
        lh_tag_template(&v, &b->cfg, b->cfg.vbr_q, h_tmpl.data());
    hipError_t e = tmpl.alloc(h_tmpl.size());
    if (e == hipSuccess)
        e = pad.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = ev[0].create();
    if (e == hipSuccess)
        e = ev[1].create();
    if (e == hipSuccess)
        e = hipMemcpy(tmpl.get(), h_tmpl.data(), h_tmpl.size(), hipMemcpyHostToDevice);
    try {
        h_pad.assign((size_t) b->B, 0);
        patched.assign((size_t) b->B, 0);
    }
    catch(const std::bad_alloc &) {
        e = hipErrorOutOfMemory;
    }
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_device_tagging: device allocation", e);
    }
    b->d_tag_tmpl = std::move(tmpl);
    b->d_tag_pad = std::move(pad);
    b->ev_tag[0] = std::move(ev[0]);
    b->ev_tag[1] = std::move(ev[1]);
    b->h_tag_pad = std::move(h_pad);
    b->tag_patched = std::move(patched);
    b->tag_p = p;
    b->dev_tag = 1;
    return 0;
}

/* HIP-event time of the tag kernel of the last lamehip_batch_encode (after lamehip_batch_sync); 0 when none ran.  Not part
 * of lamehip_batch_last_kernel_ms. */
extern "C" float
lamehip_batch_last_tag_ms(lamehip_batch * b)
{
    return b ? b->tag_ms : 0.0f;
}

/* Tag frames for an incremental batch that packs on the device (lamehip_batch_set_incremental_packing first): behind every
 * round's drain one more launch (lh_tag.hip: lh_tag_resume_kernel) moves a carry per stream on -- the music CRC over the
 * bytes that became final with the round, lh_tag_add_frame's bookkeeping over the round's records --, the final round's
 * launch makes every stream's Xing/Info + LAME frame of it, and the frames come home behind the final round's table
 * (lamehip_batch_tag_ptr / _get_tags_all).  The drains hand out what they handed out.  Only before any PCM is handed over;
 * on = 0 puts the batch back as it was. */
extern "C" int
lamehip_batch_set_incremental_tagging(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (!b->inc_pack) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_tagging: for a batch that packs its rounds on the device "
                 "(lamehip_batch_set_incremental_packing first)");
        return -1;
    }
    if (b->pcm_given || b->encoded || b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_tagging: only before any PCM is handed over");
        return -1;
    }
    if (!on || b->inc_tag) {
        b->inc_tag = on != 0 && b->inc_tag;
        return 0;
    }
    /* everything new first: a failure leaves the batch as it was */
    LhVbrTag v;
    LhTagParams p;
    LhTagPow pw;
    int const total = lh_tag_init(&v, &b->cfg);
    if (b->rate_in)
        v.samplerate_in = b->rate_in;
    lh_tag_params(&v, &b->cfg, &p);
    lh_tag_pow_table(&pw);
    size_t const room = (size_t) b->B * (size_t) (total > 0 ? total : 1);
    LhDevBuf < LhTagCarry > carry;
    LhDevBuf < LhTagPow > powers;
    LhDevBuf < unsigned char >tmpl, tags;
    LhDevBuf < int >pad;
    LhPinned < unsigned char >h_tags;
    LhEvent ev[2];
    std::vector < int >h_pad;
    std::vector < char >patched;
    std::vector < unsigned char >h_tmpl((size_t) (total > 0 ? total : 1), 0);
    if (total > 0)
        lh_tag_template(&v, &b->cfg, b->cfg.vbr_q, h_tmpl.data());
    hipError_t e = carry.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = powers.alloc(1);
    if (e == hipSuccess)
        e = tmpl.alloc(h_tmpl.size());
    if (e == hipSuccess)
        e = tags.alloc(room);
    if (e == hipSuccess)
        e = pad.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = h_tags.alloc(room);
    if (e == hipSuccess)
        e = ev[0].create();
    if (e == hipSuccess)
        e = ev[1].create();
    if (e == hipSuccess)
        e = hipMemset(carry.get(), 0, (size_t) b->B * sizeof(LhTagCarry));
    if (e == hipSuccess)
        e = hipMemset(tags.get(), 0, room);
    if (e == hipSuccess)
        e = hipMemset(pad.get(), 0, (size_t) b->B * sizeof(int));
    if (e == hipSuccess)
        e = hipMemcpy(powers.get(), &pw, sizeof(pw), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(tmpl.get(), h_tmpl.data(), h_tmpl.size(), hipMemcpyHostToDevice);
    try {
        h_pad.assign((size_t) b->B, 0);
        patched.assign((size_t) b->B, 0);
    }
    catch(const std::bad_alloc &) {
        e = hipErrorOutOfMemory;
    }
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_incremental_tagging: allocation", e);
    }
    memset(h_tags.get(), 0, room);
    b->d_tg_carry = std::move(carry);
    b->d_tg_pow = std::move(powers);
    b->d_tg_tmpl = std::move(tmpl);
    b->d_tg_tags = std::move(tags);
    b->d_tg_pad = std::move(pad);
    b->h_tg_tags = std::move(h_tags);
    b->ev_tg[0] = std::move(ev[0]);
    b->ev_tg[1] = std::move(ev[1]);
    b->h_tg_pad = std::move(h_pad);
    b->tg_patched = std::move(patched);
    b->tg_p = p;
    b->tg_have = 0;
    b->tg_ran = 0;
    b->inc_tag = 1;
    return 0;
}

/* the tag frame's length for the batch's settings; 0 when the tag does not fit a frame, or the switch is off */
extern "C" int
lamehip_batch_tag_size(lamehip_batch * b)
{
    return (b && b->inc_tag) ? b->tg_p.total : 0;
}

/* stream s's tag frame is there: the round that ended it -- lamehip_batch_finish, or the one behind
 * lamehip_batch_end_stream -- has brought it home (a batch whose tag does not fit a frame has none to bring) */
static int
batch_tag_there(const lamehip_batch * b, int s)
{
    if (!b->incremental || b->slot.empty())
        return 0;
    return b->tg_p.total > 0 ? (b->tg_have && b->tg_has[(size_t) s]) : (b->finished || b->slot[(size_t) s] == LH_SLOT_ENDED);
}

/* who: one of the tag getters of an incremental batch; s: the stream it asks for, or -1: any */
static int
batch_tags_ready(lamehip_batch * b, const char *who, int s)
{
    int     there = 0;
    if (!b)
        return -1;
    if (!b->inc_tag) {
        snprintf(g_err, sizeof(g_err), "%s: lamehip_batch_set_incremental_tagging is not on", who);
        return -1;
    }
    for (int i = 0; i < b->B && !there; i++)
        there = (s < 0 || s == i) && batch_tag_there(b, i);
    if (!there) {
        snprintf(g_err, sizeof(g_err), "%s: an incremental batch's tag frames exist after lamehip_batch_finish", who);
        return -1;
    }
    return 0;
}

/* stream s's frame in the pinned buffer, its radio gain put in (once) when the batch measured one round by round; returns
 * its length or a negative code */
static long
batch_tag_at(lamehip_batch * b, int s, unsigned char **at)
{
    int const total = b->tg_p.total;
    *at = nullptr;
    if (total <= 0)
        return 0;
    if (b->h_dr_rows.get()[s].status != 0) {
        snprintf(g_err, sizeof(g_err), "device bit packer reported status %d for stream %d", b->h_dr_rows.get()[s].status, s);
        return LAMEHIP_ERR_PAYLOAD;
    }
    *at = b->h_tg_tags.get() + (size_t) s * (size_t) total;
    if (b->inc_rg && b->rg_final[(size_t) s] && !b->tg_patched[(size_t) s]) {
        lh_tag_patch_gain(*at, b->tg_p.at, b->rg_tenths[(size_t) s]);
        b->tg_patched[(size_t) s] = 1;
    }
    return total;
}

/* stream s's final tag frame in the batch's pinned buffer (valid until lamehip_batch_reset): returns its length, or a
 * negative code */
extern "C" long
lamehip_batch_tag_ptr(lamehip_batch * b, int s, const unsigned char **frame)
{
    unsigned char *at = nullptr;
    if (!b || s < 0 || s >= b->B || !frame || batch_tags_ready(b, "lamehip_batch_tag_ptr", s) != 0)
        return -1;
    long const n = batch_tag_at(b, s, &at);
    *frame = at;
    return n;
}

/* all streams' tag frames: stream s at out + s * out_stride, sizes[s] = bytes or a negative code */
extern "C" int
lamehip_batch_get_tags_all(lamehip_batch * b, unsigned char *out, long out_stride, long *sizes)
{
    int     bad = 0;
    if (!out || !sizes || batch_tags_ready(b, "lamehip_batch_get_tags_all", -1) != 0)
        return -1;
    for (int s = 0; s < b->B; s++) {
        unsigned char *at = nullptr;
        /* (a stream that has not ended has no frame yet: a negative size, and not an error of the call) */
        if (!batch_tag_there(b, s)) {
            sizes[s] = -1;
            continue;
        }
        long    n = b->tg_p.total > out_stride ? -1 : batch_tag_at(b, s, &at);
        sizes[s] = n;
        if (n < 0)
            bad++;
        else if (n > 0)
            memcpy(out + (size_t) s * (size_t) out_stride, at, (size_t) n);
    }
    return bad ? -1 : 0;
}

/* Device tagging: the radio gain into stream s's image (tag frame first), which the kernel wrote with the field zero -- the
 * window sums become a gain on the host (batch_gain_fetch) --: the two bytes of the field, and the frame's own CRC over
 * them again (lh_tag.h).  *done (the image in the pinned buffer): once per stream and launch. */
static int
batch_image_gain(lamehip_batch * b, int s, unsigned char *image, char *done)
{
    LhVbrTag v;
    if (b->tag_room <= 0 || b->nframes[(size_t) s] == 0 || (done && *done))
        return 0;
    memset(&v, 0, sizeof(v));
    if (batch_tag_gain(b, s, &v) != 0)
        return LAMEHIP_ERR_DEVICE;
    if (v.radio_gain_on)
        lh_tag_patch_gain(image, b->tag_p.at, v.radio_gain);
    if (done)
        *done = 1;
    return 0;
}

/* who: one of the image getters of a batch whose last launch wrote the tag frames */
static int
batch_images_ready(lamehip_batch * b, const char *who)
{
    if (!b || !b->encoded || !b->dev_pack)
        return -1;
    if (!b->tagged) {
        snprintf(g_err, sizeof(g_err), "%s: no lamehip_batch_encode with lamehip_batch_set_device_tagging on has run", who);
        return -1;
    }
    return 0;
}

/* stream s's finished file image -- tag frame, then audio -- in the batch's pinned buffer (valid until the batch is encoded
 * again): returns its length, or a negative code.  Waits for lamehip_batch_fetch, like lamehip_batch_bytes_ptr. */
extern "C" long
lamehip_batch_image_ptr(lamehip_batch * b, int s, const unsigned char **image)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    const unsigned char *audio = nullptr;
    if (!b || s < 0 || s >= b->B || !image || batch_images_ready(b, "lamehip_batch_image_ptr") != 0)
        return -1;
    long const n = lamehip_batch_bytes_ptr(b, s, &audio);
    if (n < 0)
        return n;
    unsigned char *const at = b->h_bytes.get() + b->bytes_off[(size_t) s] - b->tag_room;
    if (batch_image_gain(b, s, at, b->tag_room > 0 ? &b->tag_patched[(size_t) s] : nullptr) != 0)
        return LAMEHIP_ERR_DEVICE;
    *image = at;
    return n + b->tag_room;
}

/* all streams' file images: stream s at out + s * out_stride, sizes[s] = bytes or a negative code */
extern "C" int
lamehip_batch_get_images_all(lamehip_batch * b, unsigned char *out, long out_stride, long *sizes)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int     bad = 0;
    if (!out || !sizes || batch_images_ready(b, "lamehip_batch_get_images_all") != 0)
        return -1;
    if (lamehip_batch_fetch(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    HIPCHK(hipStreamSynchronize(b->down_stream));
    for (int s = 0; s < b->B; s++) {
        long    n = (b->nframes[(size_t) s] == 0) ? 0 : (long) b->h_sum.get()[2 * s];
        unsigned char *const at = b->h_bytes.get() + b->bytes_off[(size_t) s] - b->tag_room;
        if (b->h_sum.get()[2 * s + 1] != 0)
            n = LAMEHIP_ERR_PAYLOAD;
        else if (n + b->tag_room > out_stride)
            n = -1;
        else if (batch_image_gain(b, s, at, b->tag_room > 0 ? &b->tag_patched[(size_t) s] : nullptr) != 0)
            n = LAMEHIP_ERR_DEVICE;
        else
            n += b->tag_room;
        sizes[s] = n;
        if (n < 0)
            bad++;
        else if (n > 0)
            memcpy(out + (size_t) s * (size_t) out_stride, at, (size_t) n);
    }
    return bad ? -1 : 0;
}

/* Device rate conversion (a batch whose input rate differs from the encoder's): the input stays s16, in a pool at the
 * input rate that takes PCM the way a batch without conversion does -- pinned mirror, device-resident input --, and
 * lamehip_batch_encode converts it into the float pool with a kernel (lh_resample_dev.hip) in front of the analysis
 * kernels.  Only before any PCM is handed over; off (the default): lamehip_batch_set_pcm converts on the host. */
extern "C" int
lamehip_batch_set_device_resampling(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (!b->rate_in) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_device_resampling: this batch does not convert (input rate = output rate)");
        return -1;
    }
    if (b->pcm_given || b->encoded || b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_device_resampling: only before any PCM is handed over");
        return -1;
    }
    if (!on && b->stype != LH_PCM_S16) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_device_resampling: the host converter takes s16 only, this batch's sample type is not");
        return -1;
    }
    if (!on || b->dev_rs) {
        b->dev_rs = on != 0 && b->dev_rs;
        b->inc_rs = b->inc_rs && b->dev_rs;     /* (round-by-round conversion is the device converter's) */
        return 0;
    }
    /* everything new first: a failure leaves the batch as it was */
    lh_rs_init(b->rs, b->rate_in, b->cfg.samplerate);
    int const rows = 2 * b->rs->phases + 1;
    size_t const pool = (size_t) b->B * 2 * (size_t) b->cap * sizeof(int16_t);
    LhDevBuf < int16_t > pcm;
    LhDevBuf < float >bank;
    LhDevBuf < LhRsStream > streams;
    LhEvent ev[2];
    std::vector < float >h_bank((size_t) rows * LH_RS_ROW, 0.0f);
    for (int k = 0; k < rows; k++)
        memcpy(&h_bank[(size_t) k * LH_RS_ROW], b->rs->bank[k], (size_t) (b->rs->taps + 1) * sizeof(float));
    hipError_t e = pcm.alloc(pool / sizeof(int16_t));
    if (e == hipSuccess)
        e = bank.alloc(h_bank.size());
    if (e == hipSuccess)
        e = streams.alloc((size_t) b->B);
    if (e == hipSuccess)
        e = ev[0].create();
    if (e == hipSuccess)
        e = ev[1].create();
    if (e == hipSuccess)
        e = hipMemset(pcm.get(), 0, pool);
    if (e == hipSuccess)
        e = hipMemcpy(bank.get(), h_bank.data(), h_bank.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_device_resampling: device allocation", e);
    }
    b->d_pcm = std::move(pcm);  /* (in place of the one-sample placeholder of a batch that converts on the host) */
    b->d_rs_bank = std::move(bank);
    b->d_rs_streams = std::move(streams);
    b->ev_rs[0] = std::move(ev[0]);
    b->ev_rs[1] = std::move(ev[1]);
    lh_rs_trunk_init(&b->trunk, fs_of(b->cfg), mfn_of(b->cfg));
    b->len_in.assign((size_t) b->B, 0);
    b->tail.assign((size_t) b->B, std::vector < LhRsBlock > ());
    b->rs_dirty.assign((size_t) b->B, 0);
    b->dev_rs = 1;
    return 0;
}

/* Incremental use of a batch that converts on the device (lamehip_batch_set_device_resampling first): the appends plan the
 * conversion call by call, as the reference converts when lame_encode_buffer is called with the same chunks, and every round
 * converts what was appended since the last (lh_resample_dev.hip: lh_resample_tiles_kernel).  Only before any PCM is handed
 * over; until the first append the batch still takes whole streams (lamehip_batch_set_pcm ... lamehip_batch_encode). */
extern "C" int
lamehip_batch_set_incremental_resampling(lamehip_batch * b, int on)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (!b->rate_in || !b->dev_rs) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_resampling: for a batch that converts the sample rate on the device "
                 "(lamehip_batch_set_device_resampling first)%s", b->rate_in ? "" : ", this batch does not convert");
        return -1;
    }
    if (b->pcm_given || b->encoded || b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_incremental_resampling: only before any PCM is handed over");
        return -1;
    }
    if (!on || b->inc_rs) {
        b->inc_rs = on != 0 && b->inc_rs;
        return 0;
    }
    /* everything new first: a failure leaves the batch as it was */
    LhDevBuf < LhRsTile > tiles;
    LhDevBuf < long long >lens;
    std::vector < LhRsCursor > cur;
    std::vector < long long >conv, h_lens;
    hipError_t e = tiles.alloc(4096);
    if (e == hipSuccess)
        e = lens.alloc((size_t) b->B);
    try {
        LhRsCursor first;
        lh_rs_cursor_init(&first);
        cur.assign((size_t) b->B, first);
        conv.assign((size_t) b->B, 0);
        h_lens.assign((size_t) b->B, 0);
    }
    catch(const std::bad_alloc &) {
        e = hipErrorOutOfMemory;
    }
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_incremental_resampling: allocation", e);
    }
    b->d_tiles = std::move(tiles);
    b->d_rs_lens = std::move(lens);
    b->rs_cur = std::move(cur);
    b->rs_conv = std::move(conv);
    b->h_rs_lens = std::move(h_lens);
    b->h_tiles.clear();
    b->inc_capf = b->capf;
    {
        /* LAMEHIP_INC_RS_ROOM=n, looked at here: the appends count the float pool as n converted samples per stream, no more
         * than it has (test aid: the pool's own margin, 4 * 1152 + 64, holds the flush of every stream that fits the input
         * capacity, so the appends' second refusal needs a smaller figure to be met) */
        const char *e = getenv("LAMEHIP_INC_RS_ROOM");
        long const room = e ? strtol(e, nullptr, 10) : 0;
        if (room > 0 && room < b->capf)
            b->inc_capf = room;
    }
    b->inc_rs = 1;
    return 0;
}

/* ---- streams at input rates of their own (lamehip_batch_set_stream_in_samplerate) ---- */

/* A rate is accepted when the library's own host init resolves this batch's records again for it: the handle's settings with
 * in = hz and the batch's output rate given explicitly.  The records are compared whole -- the input rate is in neither of
 * them --; nothing here reasons about which setting might matter.  0, -1 with a message that names what differs, or
 * LAMEHIP_ERR_DEVICE. */
static int
batch_rate_resolves(const lamehip_batch * b, const char *who, int hz)
{
    LhUserParams p = b->user_p;
    LhConfig cfg;
    LhInitAux aux;
    int     rc = 0;
    LhTables *tab = (LhTables *) malloc(sizeof(LhTables));
    if (!tab) {
        snprintf(g_err, sizeof(g_err), "%s: out of memory (tables)", who);
        return LAMEHIP_ERR_DEVICE;
    }
    p.samplerate = hz;
    p.samplerate_out = b->cfg.samplerate;
    if (lh_config_resolve(&p, &cfg, &aux) != 0 || lh_tables_build(&cfg, &aux, tab) != 0) {
        snprintf(g_err, sizeof(g_err), "%s: the batch's settings do not resolve for %d Hz in, %d Hz out", who, hz, b->cfg.samplerate);
        rc = -1;
    }
    else {
        const unsigned char *x = (const unsigned char *) &cfg, *y = (const unsigned char *) &b->cfg;
        size_t  at;
        for (at = 0; at < sizeof(LhConfig) && x[at] == y[at]; at++);
        if (at < sizeof(LhConfig)) {
            snprintf(g_err, sizeof(g_err), "%s: at %d Hz in (%d Hz out) the settings resolve to another LhConfig than the batch's: byte %zu "
                     "differs", who, hz, b->cfg.samplerate, at);
            rc = -1;
        }
        x = (const unsigned char *) tab;
        y = (const unsigned char *) b->tab;
        for (at = 0; rc == 0 && at < sizeof(LhTables) && x[at] == y[at]; at++);
        if (rc == 0 && at < sizeof(LhTables)) {
            snprintf(g_err, sizeof(g_err), "%s: at %d Hz in (%d Hz out) the settings resolve to other LhTables than the batch's: byte %zu "
                     "differs", who, hz, b->cfg.samplerate, at);
            rc = -1;
        }
    }
    free(tab);
    return rc;
}

/* The class of input rate hz, made on first use: its converter for the plans, its bank in HBM, its record in the class table.
 * The first class made brings the table and the room for all banks (one allocation, class 0's bank copied into it).
 * Everything is allocated first: a failure returns LAMEHIP_ERR_DEVICE and leaves the batch as it was; -1: refused. */
static int
batch_rate_class(lamehip_batch * b, const char *who, int hz, int *cls)
{
    size_t const bank_floats = (size_t) (2 * LH_RS_MAXPHASES + 1) * LH_RS_ROW;
    int const ncls = b->rs_ncls ? b->rs_ncls : 1;
    bool const first = b->rs_ncls == 0;
    int     rc;
    *cls = 0;
    if (hz == b->rate_in)
        return 0;
    for (int c = 1; c < b->rs_ncls; c++)
        if (b->rs_cls[c]->rate_in == hz) {
            *cls = c;
            return 0;
        }
    if (ncls >= LH_RS_CLASSES_MAX) {
        snprintf(g_err, sizeof(g_err), "%s: this batch has had %d distinct input rates already (LH_RS_CLASSES_MAX), %d Hz would be one more",
                 who, ncls, hz);
        return -1;
    }
    if ((rc = batch_rate_resolves(b, who, hz)) != 0)
        return rc;
    LhResampler *r = (LhResampler *) malloc(sizeof(LhResampler));
    LhDevBuf < float >banks;
    LhDevBuf < LhRsClass > classes;
    std::vector < int >scls;
    std::vector < float >h_bank;
    LhRsClass rec[2];
    hipError_t e = r ? hipSuccess : hipErrorOutOfMemory;
    memset(rec, 0, sizeof(rec));
    try {
        if (first)
            scls.assign((size_t) b->B, 0);
        h_bank.assign(bank_floats, 0.0f);
    }
    catch(const std::bad_alloc &) {
        e = hipErrorOutOfMemory;
    }
    if (e == hipSuccess) {
        if (lh_rs_needed(hz, b->cfg.samplerate)) {
            lh_rs_init(r, hz, b->cfg.samplerate);
            for (int k = 0; k < 2 * r->phases + 1; k++)
                memcpy(&h_bank[(size_t) k * LH_RS_ROW], r->bank[k], (size_t) (r->taps + 1) * sizeof(float));
        }
        else
            lh_rs_init_identity(r, hz, b->cfg.samplerate);
        rec[1].ratio = r->ratio;
        rec[1].taps = r->taps;
        rec[1].phases = r->phases;
        rec[1].identity = lh_rs_is_identity(r);
        rec[1].bank_at = (long long) ((size_t) ncls * bank_floats);
        rec[0].ratio = b->rs->ratio;
        rec[0].taps = b->rs->taps;
        rec[0].phases = b->rs->phases;
    }
    if (e == hipSuccess && first)
        e = banks.alloc((size_t) LH_RS_CLASSES_MAX * bank_floats);
    if (e == hipSuccess && first)
        e = classes.alloc(LH_RS_CLASSES_MAX);
    float  *const d_banks = first ? banks.get() : b->d_rs_banks.get();
    LhRsClass *const d_classes = first ? classes.get() : b->d_rs_classes.get();
    if (e == hipSuccess && first)
        e = hipMemset(d_banks, 0, (size_t) LH_RS_CLASSES_MAX * bank_floats * sizeof(float));
    if (e == hipSuccess && first)
        e = hipMemset(d_classes, 0, LH_RS_CLASSES_MAX * sizeof(LhRsClass));
    if (e == hipSuccess && first)
        e = hipMemcpy(d_banks, b->d_rs_bank.get(), (size_t) (2 * b->rs->phases + 1) * LH_RS_ROW * sizeof(float), hipMemcpyDeviceToDevice);
    if (e == hipSuccess && first)
        e = hipMemcpy(d_classes, &rec[0], sizeof(LhRsClass), hipMemcpyHostToDevice);
    if (e == hipSuccess && !rec[1].identity)
        e = hipMemcpy(d_banks + (size_t) ncls * bank_floats, h_bank.data(), bank_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(d_classes + ncls, &rec[1], sizeof(LhRsClass), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        free(r);
        return set_err("lamehip_batch_set_stream_in_samplerate: allocation", e);
    }
    if (first) {
        b->d_rs_banks = std::move(banks);
        b->d_rs_classes = std::move(classes);
        b->rs_scls = std::move(scls);
        b->rs_cls[0] = b->rs;
        b->h_rs_cls[0] = rec[0];
    }
    b->rs_cls[ncls] = r;
    b->h_rs_cls[ncls] = rec[1];
    b->rs_ncls = ncls + 1;
    *cls = ncls;
    return 0;
}

/* Stream s arrives at hz (include/lamehip.h has the contract): from here on its appends and its flush are planned with the
 * converter of that rate's class -- or not converted at all, where the reference would not --, and its tag frame names the
 * rate.  For a batch that converts round by round, and a stream that has nothing appended yet. */
extern "C" int
lamehip_batch_set_stream_in_samplerate(lamehip_batch * b, int s, int hz)
{
    static const char who[] = "lamehip_batch_set_stream_in_samplerate";
    LhDeviceScope const on_device(b ? b->device : -1);
    int     rc, cls = 0;
    if (!b || s < 0 || s >= b->B) {
        snprintf(g_err, sizeof(g_err), "%s: no such stream", who);
        return -1;
    }
    if (hz <= 0) {
        snprintf(g_err, sizeof(g_err), "%s: an input rate of %d Hz", who, hz);
        return -1;
    }
    if (!b->inc_rs) {
        snprintf(g_err, sizeof(g_err), "%s: for a batch that converts the sample rate round by round (lamehip_batch_set_device_resampling, "
                 "then lamehip_batch_set_incremental_resampling)", who);
        return -1;
    }
    if (b->finished) {
        snprintf(g_err, sizeof(g_err), "%s: the batch is finished (lamehip_batch_reset starts it over)", who);
        return -1;
    }
    if (b->incremental
        && (b->slot[(size_t) s] != LH_SLOT_LIVE || b->fed[(size_t) s] + b->staged[(size_t) s] > 0 || b->rs_cur[(size_t) s].in_at > 0)) {
        snprintf(g_err, sizeof(g_err), "%s: stream %d %s: a stream's rate is stated before its first sample (in a fresh batch, after "
                 "lamehip_batch_reset or lamehip_batch_restart_stream)", who, s,
                 b->slot[(size_t) s] != LH_SLOT_LIVE ? "has ended" : "has samples already");
        return -1;
    }
    if ((rc = batch_rate_class(b, who, hz, &cls)) != 0)
        return rc;
    if (!b->rs_scls.empty())
        b->rs_scls[(size_t) s] = cls;
    return 0;
}

/* the input rate of stream s: the batch's own when none was stated; -1: no such stream */
extern "C" int
lamehip_batch_stream_in_samplerate(lamehip_batch * b, int s)
{
    if (!b || s < 0 || s >= b->B) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_stream_in_samplerate: no such stream");
        return -1;
    }
    int const cls = batch_stream_cls(b, s);
    return cls ? b->rs_cls[cls]->rate_in : b->rate_in ? b->rate_in : b->cfg.samplerate;
}

/* The sample type of the input pool (LAMEHIP_PCM_*), only before any PCM is handed over.  Other than s16 the batch gets an
 * input pool of that element type in place of the s16 pool and -- unless it converts the rate, which brings one -- a float
 * pool of the same geometry for the kernels to read. */
extern "C" int
lamehip_batch_set_sample_type(lamehip_batch * b, int type)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (type < 0 || type >= LH_PCM_TYPES) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_sample_type: no sample type %d", type);
        return -1;
    }
    if (b->pcm_given || b->encoded || b->incremental) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_sample_type: only before any PCM is handed over");
        return -1;
    }
    if (type != LH_PCM_S16 && b->rate_in && !b->dev_rs) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_set_sample_type: a batch that converts the sample rate on the host takes s16 only "
                 "(lamehip_batch_set_device_resampling first)");
        return -1;
    }
    if (type == b->stype)
        return 0;
    /* everything new first: a failure leaves the batch as it was */
    int const esz = lh_pcm_elem_size(type);
    bool const own_floats = (type != LH_PCM_S16 && !b->rate_in);
    size_t const pool = (size_t) b->B * 2 * (size_t) b->cap * (size_t) esz;
    LhDevBuf < int16_t > pcm;
    LhDevBuf < float >pcmf;
    LhDevBuf < LhInStream > streams;
    LhEvent ev[2];
    hipError_t e = pcm.alloc(pool / sizeof(int16_t));
    if (e == hipSuccess && own_floats)
        e = pcmf.alloc((size_t) b->B * 2 * (size_t) b->cap);
    if (e == hipSuccess && own_floats)
        e = streams.alloc((size_t) b->B);
    if (e == hipSuccess && own_floats)
        e = ev[0].create();
    if (e == hipSuccess && own_floats)
        e = ev[1].create();
    if (e == hipSuccess)
        e = hipMemset(pcm.get(), 0, pool);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return set_err("lamehip_batch_set_sample_type: device allocation", e);
    }
    b->d_pcm = std::move(pcm);
    b->h_pcm.release();         /* (none yet: asking for the mirror hands PCM over) */
    if (!b->rate_in) {
        b->d_pcmf = std::move(pcmf);    /* (back to s16: released) */
        b->capf = own_floats ? b->cap : 0;
        b->d_in_streams = std::move(streams);
        b->ev_in[0] = std::move(ev[0]);
        b->ev_in[1] = std::move(ev[1]);
    }
    b->in_dirty.assign((size_t) b->B, 0);
    b->stype = type;
    b->esz = esz;
    return 0;
}

/* test accessor: the float planes of stream s as the encoder reads them -- the converted signal (after
 * lamehip_batch_set_pcm when the host converts, after lamehip_batch_encode when the device does), or what the ingest made
 * of a typed stream (after lamehip_batch_encode); returns the length, or a negative code */
extern "C" long
lamehip_batch_get_converted(lamehip_batch * b, int s, float *l, float *r, long cap)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b || s < 0 || s >= b->B || !batch_reads_floats(b) || !l || !r)
        return -1;
    if (b->dev_rs ? b->rs_dirty[(size_t) s] : (b->stype != LH_PCM_S16 && b->in_dirty[(size_t) s])) {
        snprintf(g_err, sizeof(g_err), "lamehip_batch_get_converted: stream %d has not been converted yet (lamehip_batch_encode)", s);
        return -1;
    }
    /* (an incremental typed batch: the float planes up to what has reached the pool) */
    long const n = !b->incremental ? b->len[(size_t) s] : b->inc_rs ? (long) b->rs_conv[(size_t) s] : b->fed[(size_t) s];
    if (n > cap)
        return -1;
    HIPCHK(hipStreamSynchronize(b->stream));
    if (n > 0) {
        HIPCHK(hipMemcpy(l, b->d_pcmf.get() + ((size_t) s * 2) * (size_t) b->capf, (size_t) n * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(r, b->d_pcmf.get() + ((size_t) s * 2 + 1) * (size_t) b->capf, (size_t) n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return n;
}

/* HIP-event time of the device conversion of the last lamehip_batch_encode (after lamehip_batch_sync); 0 when none ran */
extern "C" float
lamehip_batch_last_resample_ms(lamehip_batch * b)
{
    return b ? b->rs_ms : 0.0f;
}

/* HIP-event time of the ingest kernel of the last lamehip_batch_encode (after lamehip_batch_sync); 0 when none ran */
extern "C" float
lamehip_batch_last_ingest_ms(lamehip_batch * b)
{
    return b ? b->in_ms : 0.0f;
}

/* bytes of one stream as the device packed them (audio frames incl. the final padding, no tag) */
extern "C" long
lamehip_batch_get_bytes(lamehip_batch * b, int s, unsigned char *out, long out_size)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    LhStreamState st;
    long    n;
    if (!b || s < 0 || s >= b->B || !b->encoded || !b->dev_pack)
        return -1;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy(&st, b->d_state.get() + s, sizeof(st), hipMemcpyDeviceToHost));
    if (st.status != 0) {
        snprintf(g_err, sizeof(g_err), "device bit packer reported status %d for stream %d", st.status, s);
        return LAMEHIP_ERR_PAYLOAD;
    }
    n = (long) st.em_next_header;
    if (b->nframes[(size_t) s] == 0)
        n = 0;
    if (n > out_size)
        return -1;
    if (n > 0)
        HIPCHK(hipMemcpy(out, b->d_bytes.get() + b->bytes_off[(size_t) s], (size_t) n, hipMemcpyDeviceToHost));
    return n;
}

/* device-packed stream as a complete file image: the final Xing/Info + LAME tag frame, then the audio
 * frames.  The tag's bookkeeping (frame count, bitrate table of contents, music CRC, mode extension of
 * the last frame) is read back from the frame headers of the bytes themselves. */
extern "C" long
lamehip_batch_get_bytes_tagged(lamehip_batch * b, int s, unsigned char *out, long out_size)
{
    LhVbrTag v;
    int     total, last_mode_ext = 0;
    long    k, pos = 0;
    if (!b || s < 0 || s >= b->B || !b->encoded || !b->dev_pack)
        return -1;
    if (b->tagged && b->tag_room > 0) {
        /* device tagging: the tag frame lies in front of the bytes in HBM; only the gain is the host's */
        LhDeviceScope const on_device(b->device);
        if (out_size < b->tag_room)
            return -1;
        k = lamehip_batch_get_bytes(b, s, out + b->tag_room, out_size - b->tag_room);
        if (k < 0)
            return k;
        HIPCHK(hipMemcpy(out, b->d_bytes.get() + b->bytes_off[(size_t) s] - b->tag_room, (size_t) b->tag_room, hipMemcpyDeviceToHost));
        if (batch_image_gain(b, s, out, nullptr) != 0)
            return LAMEHIP_ERR_DEVICE;
        return k + b->tag_room;
    }
    total = lh_tag_init(&v, &b->cfg);
    if (b->rate_in)
        v.samplerate_in = b->rate_in;
    if (out_size < total)
        return -1;
    if (batch_tag_gain(b, s, &v) != 0)
        return LAMEHIP_ERR_DEVICE;
    k = lamehip_batch_get_bytes(b, s, out + total, out_size - total);
    if (k < 0 || total == 0)
        return k;
    while (pos + 4 <= k) {
        const unsigned char *h = out + total + pos;
        int const bi = h[2] >> 4, pad = (h[2] >> 1) & 1;
        int const kbps = lh_tag_kbps(b->cfg.version, bi);
        int const size = (b->cfg.version + 1) * 72000 * kbps / b->cfg.samplerate + pad;
        if (h[0] != 0xff || (h[1] & 0xe0) != 0xe0 || kbps <= 0 || size <= 0) {
            snprintf(g_err, sizeof(g_err), "device-packed stream %d: lost frame sync at byte %ld", s, pos);
            return LAMEHIP_ERR_PAYLOAD;
        }
        lh_tag_add_frame(&v, kbps);
        last_mode_ext = (h[3] >> 4) & 3;
        pos += size;
    }
    lh_tag_crc(&v, out + total, k);
    if (lh_tag_frame(&v, &b->cfg, b->cfg.vbr_q, batch_padding(b, s), last_mode_ext, out, total) != total)
        memset(out, 0, (size_t) total);         /* no frames: the reference leaves the placeholder */
    return k + total;
}

/* all streams: stream s at out + s * out_stride, sizes[s] = bytes or a negative code */
extern "C" int
lamehip_batch_get_bytes_all(lamehip_batch * b, unsigned char *out, long out_stride, long *sizes)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int     bad = 0;
    if (!b || !b->encoded || !b->dev_pack || !out || !sizes)
        return -1;
    if (lamehip_batch_fetch(b) != 0)
        return LAMEHIP_ERR_DEVICE;
    HIPCHK(hipStreamSynchronize(b->down_stream));
    for (int s = 0; s < b->B; s++) {
        long    n = (b->nframes[(size_t) s] == 0) ? 0 : (long) b->h_sum.get()[2 * s];
        if (b->h_sum.get()[2 * s + 1] != 0)
            n = LAMEHIP_ERR_PAYLOAD;
        else if (n > out_stride)
            n = -1;
        sizes[s] = n;
        if (n < 0)
            bad++;
        else if (n > 0)
            memcpy(out + (size_t) s * (size_t) out_stride, b->h_bytes.get() + b->bytes_off[(size_t) s], (size_t) n);
    }
    return bad ? -1 : 0;
}

/* The buffers a launch of the batch's present streams needs -- payload, the analysis kernels' pool (split pipeline), the byte
 * pool of the device packer -- allocated now instead of by the first lamehip_batch_encode (81 GB of pool at 1024 x 60 s: a
 * caller that times its first launch calls this first). */
extern "C" int
lamehip_batch_reserve(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    long long total = 0, bytes_total = 0;
    if (!b)
        return -1;
    if (b->incremental)
        return 0;               /* (incremental batches launch what has arrived: sized per launch) */
    for (int s = 0; s < b->B; s++) {
        total += b->nframes[(size_t) s];
        bytes_total += batch_tag_room(b) + batch_stream_bytes(b, s);
    }
    {
        int const rc = batch_pools_reserve(b, total, bytes_total);
        if (rc)
            return rc;
    }
    if (b->split && total > 0 && !batch_window_env())
        (void) batch_mid_reserve(b, total);     /* (no room: the launch will run in windows, or take the fused kernel) */
    return 0;
}

extern "C" int
lamehip_batch_sync(lamehip_batch * b)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b)
        return -1;
    if (b->ev_wait && b->launched) {
        /* The wait for the launch: the runtime's own waits spin on the stream's signal whatever the event's flags say
         * (measured: one CPU per rank for the whole launch), so the event is polled between short sleeps -- at most 100 us
         * late on a launch of tens to hundreds of milliseconds, and the CPU is free meanwhile. */
        hipError_t q;
        struct timespec nap = { 0, 100000 };
        while ((q = hipEventQuery(b->ev_wait)) == hipErrorNotReady)
            nanosleep(&nap, nullptr);
        if (q != hipSuccess)
            return set_err("hipEventQuery", q);
    }
    if (b->up_stream) {
        HIPCHK(hipStreamSynchronize(b->up_stream));
        HIPCHK(hipStreamSynchronize(b->down_stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    if (b->encoded) {
        float   ms = 0;
        b->rs_ms = 0;
        if (b->rs_ran && hipEventElapsedTime(&b->rs_ms, b->ev_rs[0], b->ev_rs[1]) != hipSuccess) {
            (void) hipGetLastError();
            b->rs_ms = 0;
        }
        b->in_ms = 0;
        if (b->in_ran && hipEventElapsedTime(&b->in_ms, b->ev_in[0], b->ev_in[1]) != hipSuccess) {
            (void) hipGetLastError();
            b->in_ms = 0;
        }
        b->rg_ms = 0;
        if (b->rg_ran && hipEventElapsedTime(&b->rg_ms, b->ev_rg[0], b->ev_rg[1]) != hipSuccess) {
            (void) hipGetLastError();
            b->rg_ms = 0;
        }
        b->tag_ms = 0;
        if (b->tag_ran && hipEventElapsedTime(&b->tag_ms, b->ev_tag[0], b->ev_tag[1]) != hipSuccess) {
            (void) hipGetLastError();
            b->tag_ms = 0;
        }
        if (hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess)
            b->last_ms = ms;
        b->part_ms[0] = b->part_ms[1] = b->part_ms[2] = 0;
        if (b->last_split && b->last_windows > 1) {
            /* a launch in windows: the three parts summed over the windows (a window ends where the next one starts) */
            for (int k = 0; k < b->last_windows; k++) {
                hipEvent_t const e0 = b->ev_win[3 * (size_t) k], e1 = b->ev_win[3 * (size_t) k + 1], e2 = b->ev_win[3 * (size_t) k + 2];
                hipEvent_t const e3 = (k + 1 < b->last_windows) ? (hipEvent_t) b->ev_win[3 * (size_t) k + 3] : (hipEvent_t) b->ev1;
                float   a = 0, s_ = 0, q = 0;
                if (hipEventElapsedTime(&a, e0, e1) != hipSuccess || hipEventElapsedTime(&s_, e1, e2) != hipSuccess
                    || hipEventElapsedTime(&q, e2, e3) != hipSuccess) {
                    (void) hipGetLastError();
                    b->part_ms[0] = b->part_ms[1] = b->part_ms[2] = 0.0f;
                    break;
                }
                b->part_ms[0] += a;
                b->part_ms[1] += s_;
                b->part_ms[2] += q;
            }
        }
        else if (b->last_split) {
            if (hipEventElapsedTime(&b->part_ms[0], b->ev0, b->ev_part[0]) != hipSuccess
                || hipEventElapsedTime(&b->part_ms[1], b->ev_part[0], b->ev_part[1]) != hipSuccess
                || hipEventElapsedTime(&b->part_ms[2], b->ev_part[1], b->ev1) != hipSuccess) {
                (void) hipGetLastError();
                b->part_ms[0] = b->part_ms[1] = b->part_ms[2] = 0.0f;   /* (never a stale figure of an earlier launch) */
            }
        }
    }
    return 0;
}

extern "C" float
lamehip_batch_last_kernel_ms(lamehip_batch * b)
{
    return b ? b->last_ms : 0.0f;
}

/* the last launch kernel by kernel (split pipeline): analysis kernels, sub-band kernel, encode kernel, in ms; returns 1 when
 * the launch went through the split pipeline, 0 for the fused kernel (all of lamehip_batch_last_kernel_ms is that one kernel) */
extern "C" int
lamehip_batch_last_kernel_parts_ms(lamehip_batch * b, float *parts3)
{
    if (!b || !parts3)
        return -1;
    parts3[0] = b->part_ms[0];
    parts3[1] = b->part_ms[1];
    parts3[2] = b->part_ms[2];
    return b->last_split;
}

/* sub-launches of the last launch: 1, or the number of frame windows the split pipeline worked through (batch_plan) */
extern "C" int
lamehip_batch_last_windows(lamehip_batch * b)
{
    return b ? b->last_windows : 0;
}

extern "C" int
lamehip_batch_kernel_waves(lamehip_batch * b)
{
    return b ? 2 : 0;
}

extern "C" int
lamehip_batch_get_frames(lamehip_batch * b, int s, void *frames_out, int max_frames)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int     n;
    if (!b || s < 0 || s >= b->B || !b->encoded)
        return -1;
    n = b->nframes[(size_t) s];
    if (n > max_frames)
        n = max_frames;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipMemcpy(frames_out, b->d_out.get() + b->out_off[(size_t) s], (size_t) n * sizeof(LhFrameOut),
                     hipMemcpyDeviceToHost));
    return n;
}


/* test accessor: the device packer's byte pool in HBM as the last lamehip_batch_reserve / lamehip_batch_encode left it
 * (device tagging: the tag frames' room included), and its size; NULL when there is none */
extern "C" void *
lamehip_batch_bytes_device_ptr(lamehip_batch * b, long long *size)
{
    if (size)
        *size = b ? (long long) b->d_bytes.cap() : 0;
    return b ? (void *) b->d_bytes.get() : nullptr;
}

/* debug / profiling aid: raw LhStreamState of one stream */
extern "C" int
lamehip_batch_get_state(lamehip_batch * b, int s, void *out, int size)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    if (!b || s < 0 || s >= b->B || size < (int) sizeof(LhStreamState))
        return -1;
    /* (slots restarted since the last round: their records are put back first, and the next round finds nothing owed) */
    if (!b->sl_list.empty()) {
        int const rc = batch_restart_launch(b);
        if (rc)
            return rc;
        b->sl_gap = 1;
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    batch_restart_time(b);
    HIPCHK(hipMemcpy(out, b->d_state.get() + s, sizeof(LhStreamState), hipMemcpyDeviceToHost));
    return (int) sizeof(LhStreamState);
}

/* host bit packing of one stream from its frames (already on the host) */
static long
pack_stream(const lamehip_batch * b, int s, const LhFrameOut * fr, int n, unsigned char *out, long out_size)
{
    LhBitstream bs;
    long    pos = 0;
    if (lh_bs_init(&bs) != 0)
        return -2;
    for (int i = 0; i < n; i++) {
        int     k;
        if (lh_bs_format_frame(&bs, &b->cfg, b->tab, &fr[i]) != 0) {
            snprintf(g_err, sizeof(g_err), "inconsistent device payload (packer check %d) stream %d frame %d",
                     bs.error, s, i);
            lh_bs_free(&bs);
            return LAMEHIP_ERR_PAYLOAD;
        }
        if (lh_bs_pending(&bs) > out_size - pos) {
            lh_bs_free(&bs);
            return -1;
        }
        k = lh_bs_copy(&bs, out + pos, 0);
        pos += k;
    }
    lh_bs_flush(&bs, &b->cfg, n > 0 ? &fr[n - 1] : nullptr);
    {
        int     k;
        if (lh_bs_pending(&bs) > out_size - pos) {
            lh_bs_free(&bs);
            return -1;
        }
        k = lh_bs_copy(&bs, out + pos, 0);
        pos += k;
    }
    lh_bs_free(&bs);
    return pos;
}

extern "C" long
lamehip_batch_pack(lamehip_batch * b, int s, unsigned char *out, long out_size)
{
    std::vector < LhFrameOut > fr;
    int     n;
    if (!b || s < 0 || s >= b->B || !b->encoded)
        return -1;
    n = b->nframes[(size_t) s];
    fr.resize((size_t) n);
    if (lamehip_batch_get_frames(b, s, fr.data(), n) != n)
        return LAMEHIP_ERR_DEVICE;
    return pack_stream(b, s, fr.data(), n, out, out_size);
}

/* One stream as a complete file image: the final Xing/Info + LAME tag frame followed by the audio
 * frames (what the reference's frontend leaves on disk after lame_mp3_tags_fid).  When the tag
 * does not fit the frame size the audio alone is returned, as the reference would. */
extern "C" long
lamehip_batch_pack_tagged(lamehip_batch * b, int s, unsigned char *out, long out_size)
{
    LhVbrTag v;
    std::vector < LhFrameOut > fr;
    int     n, total;
    long    k;
    if (!b || s < 0 || s >= b->B || !b->encoded)
        return -1;
    total = lh_tag_init(&v, &b->cfg);
    if (b->rate_in)
        v.samplerate_in = b->rate_in;
    if (out_size < total)
        return -1;
    if (batch_tag_gain(b, s, &v) != 0)
        return LAMEHIP_ERR_DEVICE;
    n = b->nframes[(size_t) s];
    fr.resize((size_t) n);
    if (lamehip_batch_get_frames(b, s, fr.data(), n) != n)
        return LAMEHIP_ERR_DEVICE;
    k = pack_stream(b, s, fr.data(), n, out + total, out_size - total);
    if (k < 0 || total == 0)
        return k;
    for (int i = 0; i < n; i++)
        lh_tag_add_frame(&v, lh_tag_kbps(b->cfg.version, fr[(size_t) i].bitrate_index));
    lh_tag_crc(&v, out + total, k);
    if (lh_tag_frame(&v, &b->cfg, b->cfg.vbr_q, batch_padding(b, s), n > 0 ? fr[(size_t) n - 1].mode_ext : 0,
                     out, total) != total)
        memset(out, 0, (size_t) total);         /* no frames: the reference leaves the placeholder */
    return k + total;
}

/* All streams, `nthreads' host threads: thread t takes streams t, t + nthreads, ...; each copies
 * a stream's payload D2H into its own pinned buffer and packs it (the packer is serial per
 * stream -- reference bitstream.c -- but streams are independent).  Stream s is written at
 * out + s * out_stride; sizes[s] = bytes, or a negative error code. */
extern "C" int
lamehip_batch_pack_all(lamehip_batch * b, int nthreads, unsigned char *out, long out_stride, long *sizes)
{
    LhDeviceScope const on_device(b ? b->device : -1);
    int     dev = 0, maxf = 0;
    std::atomic < int >failed(0);
    /* the first failure of any worker: its code and its message (g_err is per thread) reach the caller */
    std::mutex first_lock;
    int     first_code = 0;
    char    first_text[sizeof(g_err)] = "";
    if (!b || !b->encoded || !out || !sizes || out_stride <= 0)
        return -1;
    if (nthreads < 1)
        nthreads = 1;
    if (nthreads > b->B)
        nthreads = b->B;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(hipGetDevice(&dev));
    for (int s = 0; s < b->B; s++)
        maxf = b->nframes[(size_t) s] > maxf ? b->nframes[(size_t) s] : maxf;
    {
        std::vector < std::thread > pool;
        for (int t = 0; t < nthreads; t++)
            pool.emplace_back([=, &failed, &first_lock, &first_code, &first_text] () {
                auto note = [&](long code, const char *text) {
                    std::lock_guard < std::mutex > hold(first_lock);
                    if (first_code == 0) {
                        first_code = (int) code;
                        snprintf(first_text, sizeof(first_text), "%s", text);
                    }
                    failed = 1;
                };
                LhPinned < LhFrameOut > h;
                LhStream st;
                if (hipSetDevice(dev) != hipSuccess
                    || h.alloc((size_t) (maxf > 0 ? maxf : 1)) != hipSuccess
                    || st.create(hipStreamNonBlocking) != hipSuccess) {
                    note(LAMEHIP_ERR_DEVICE, "pack_all: a worker could not set up its device staging");
                    for (int s = t; s < b->B; s += nthreads)
                        sizes[s] = LAMEHIP_ERR_DEVICE;
                    return;
                }
                for (int s = t; s < b->B; s += nthreads) {
                    int const n = b->nframes[(size_t) s];
                    long    r;
                    if (n > 0 && (hipMemcpyAsync(h.get(), b->d_out.get() + b->out_off[(size_t) s], (size_t) n * sizeof(LhFrameOut),
                                                 hipMemcpyDeviceToHost, st) != hipSuccess
                                  || hipStreamSynchronize(st) != hipSuccess))
                    {
                        r = LAMEHIP_ERR_DEVICE;
                        snprintf(g_err, sizeof(g_err), "pack_all: copying stream %d's frames from the device failed", s);
                    }
                    else
                        r = pack_stream(b, s, h.get(), n, out + (size_t) s * (size_t) out_stride, out_stride);
                    sizes[s] = r;
                    if (r < 0) {
                        if (r == -1)
                            snprintf(g_err, sizeof(g_err), "pack_all: out_stride %ld is too small for stream %d", out_stride, s);
                        note(r, g_err);
                    }
                }
            });
        for (auto & th:pool)
            th.join();
    }
    if (failed) {
        snprintf(g_err, sizeof(g_err), "%s", first_text);
        return first_code;
    }
    return 0;
}
