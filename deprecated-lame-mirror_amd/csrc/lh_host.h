/*
 * lh_host.h -- internal host-side interfaces of liblamehip (plain C).
 */
#ifndef LH_HOST_H
#define LH_HOST_H

#include "lamehip_types.h"
#include "lh_rs_sample.h"
#include "lh_tag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what the lame_set_* calls of the public API collect before lame_init_params */
typedef struct LhUserParams {
    int     samplerate;
    int     channels;
    int     brate;               /* kbps */
    int     mode;                /* -1 = not set (joint stereo), else LH_MODE_* */
    int     quality;             /* -1 = default (3) */
    int     vbr;                 /* 0 = CBR, 1 / 4 = vbr_mt / vbr_mtrh (the same loop in the reference), 3 = ABR */
    int     vbr_q;               /* VBR quality 0..9 (lame_set_VBR_q), default 4 */
    int     samplerate_out;      /* 0 = let the encoder choose; != samplerate: the input is resampled (lh_resample.c) */
    int     abr_kbps;            /* ABR mean bitrate (lame_set_VBR_mean_bitrate_kbps), default 128 */
    /* frontend-level switches with the reference's defaults (lame.c:2280-2420) */
    int     force_ms, disable_reservoir, error_protection, copyright, original, emphasis, extension;
    int     short_blocks;        /* -1 not set, else short_block_t: 0 allowed, 1 coupled, 2 dispensed, 3 forced */
    int     strict_ISO;          /* 0 MDB_DEFAULT, 1 MDB_STRICT_ISO, 2 MDB_MAXIMUM (default) */
    int     lowpassfreq;         /* 0 = by bitrate / quality, -1 = none, else Hz */
    int     lowpasswidth;        /* -1 = default */
    float   scale, scale_left, scale_right;
    float   vbr_q_frac;          /* lame_set_VBR_quality: the fractional part of -V n.f */
    int     vbr_min_kbps, vbr_max_kbps, vbr_hard_min;   /* -b / -B / -F with VBR or ABR; 0 = not set */
    /* tuning switches of the frontend's "experimental" section, with the reference's "not set" values
     * (lame.c:2340-2400): a value the caller left alone takes the bitrate's / quality's preset value
     * (presets.c SET_OPTION) or the default lame_init_params falls back to (lame.c:1112-1180) */
    float   msfix;               /* -1 */
    int     ATHtype;             /* -1 */
    float   ATHcurve;            /* -1 */
    float   ATH_lower_db;        /* 0; lame_set_ATHlower */
    int     athaa_type;          /* -1 */
    float   athaa_sensitivity;   /* 0 */
    int     ATHonly, ATHshort, noATH;
    float   interChRatio;        /* -1 */
    int     useTemporal;         /* -1 */
    int     highpassfreq;        /* 0 = none, -1 = off */
    int     highpasswidth;       /* -1 = default */
    int     exp_nspsytune;       /* bit 1 safe joint stereo, bits 2.. the bass / alto / treble / sfb21 adjustments */
    int     experimentalY, experimentalZ;
    int     free_format;
    float   compression_ratio;   /* 0 = not set: CBR without a bitrate takes 11.025 (lame.c:622-644) */
    int     preset_kbps;         /* 0, or the bitrate lame_set_preset(8..320 / INSANE) applied its tuning row for at call time */
} LhUserParams;

/* values that only feed table generation */
typedef struct LhInitAux {
    float   lowpass1, lowpass2;
    float   attackthre, attackthre_s;
    int     vbr_q;               /* VBR_q / VBR_q_frac as psymodel_init sees them (4 / 0 for CBR) */
    float   vbr_q_frac;
    float   athaa_sensitivity;
    float   adjust_sfb21_db;     /* exp_nspsytune bits 20..25 (+ the treble adjustment), reference lame.c:1196-1203 */
    float   adjust_bass_db, adjust_alto_db, adjust_treble_db;    /* bits 2..7, 8..13, 14..19 */
    int     athaa_type;          /* ATH->use_adjust: 3 unless lame_set_athaa_type said otherwise */
    float   highpass1, highpass2;        /* edges of the polyphase high-pass, as fractions of the Nyquist rate */
    int     samplerate_in;       /* the caller's rate; LhConfig.samplerate is the output rate */
} LhInitAux;

void    lh_params_default(LhUserParams * p);
int     lh_config_resolve(const LhUserParams * p, LhConfig * c, LhInitAux * aux);
float   lh_abr_preset_scale(int kbps);
int     lh_tables_build(LhConfig * c, const LhInitAux * aux, LhTables * t);

/* number of MP3 frames the reference produces for n input samples per channel
 * when followed by lame_encode_flush (reference lame.c:1671-1775, 2041-2120) */
int     lh_total_frames(long nsamples);
int     lh_total_frames_fs(long nsamples, int samples_per_frame);       /* 576 for MPEG-2 / 2.5 */
const int16_t *lh_bitrate_row(int version);     /* the frame sizes' kb/s of an MPEG version (lh_host_init.c) */

/* ------------------------------------------------------------------ */
/* serial bit packer (reference bitstream.c), host only                */
#define LH_MAX_HEADER_BUF 256
#define LH_MAX_HEADER_LEN 40
#define LH_BS_BUFSIZE (16384 + 147456)   /* LAME_MAXMP3BUFFER, reference lame.h */

/* a frame header + side information waiting for its place in the byte stream */
typedef struct LhQueuedHeader {
    int     due;                 /* stream position (bits) at which it is inserted */
    unsigned char bytes[LH_MAX_HEADER_LEN];
} LhQueuedHeader;

typedef struct LhBitstream {
    unsigned char *buf;          /* finished bytes not yet handed to the caller */
    int     buf_size;
    int     fill;                /* how many there are */
    unsigned long long acc;      /* main-data bits on their way into whole bytes */
    int     acc_bits;
    int     stream_bits;         /* bits in the stream so far (whole bytes, headers included) */
    LhQueuedHeader queue[LH_MAX_HEADER_BUF];
    int     q_in, q_out;         /* ring: next free slot, oldest waiting header */
    int     hdr_len;             /* header + side information, bytes */
    int     stuff_bit;
    int     main_data_begin;     /* packer's own running value, cross-checked with the device's */
    int     error;
} LhBitstream;

int     lh_bs_init(LhBitstream * bs);
int     lh_bs_init_sized(LhBitstream * bs, int size);
/* CRC-16 of a frame's protected part: header bytes 2..3 and 6..len-1 (ISO/IEC 11172-3 2.4.3.1; reference
 * bitstream.c:304-318 CRC_writeheader); the caller stores it big-endian in bytes 4..5 */
unsigned lh_header_crc(const unsigned char *h, int len);
void    lh_bs_free(LhBitstream * bs);
/* appends one frame; returns 0, or <0 when the device payload is inconsistent */
int     lh_bs_format_frame(LhBitstream * bs, const LhConfig * c, const LhTables * t,
                           const LhFrameOut * fo);
void    lh_bs_flush(LhBitstream * bs, const LhConfig * c, const LhFrameOut * last);
/* moves the finished bytes out (reference copy_buffer); -1 if size!=0 and too small */
int     lh_bs_copy(LhBitstream * bs, unsigned char *out, int size);
/* bytes waiting to be copied out */
int     lh_bs_pending(const LhBitstream * bs);


/* ---- Xing/Info + LAME tag bookkeeping (lh_vbrtag.c; reference VbrTag.c) ---- */
#define LH_LAMEHEADERSIZE (4 + 4 + 4 + 4 + 100 + 4 + 9 + 1 + 1 + 8 + 1 + 1 + 3 + 1 + 1 + 2 + 4 + 2 + 2)
#define LH_TAG_BAG LH_TAG_BAG_SIZE      /* 400 (lh_tag.h) */
typedef struct LhVbrTag {
    int     enabled;
    int     total_frame_size;
    int     sum, seen, want, pos, size;
    int     bag[LH_TAG_BAG];
    unsigned num_frames;
    unsigned long bytes_written;
    uint16_t music_crc;
    int     samplerate_in;       /* source rate for the tag's info byte (lh_tag_init: the output rate) */
    int     radio_gain_on, radio_gain;   /* lame_set_findReplayGain: the title's gain in tenths of a dB */
    int     nogap_total, nogap_current;  /* the frontend's --nogap: this title's place in the set */
} LhVbrTag;

int     lh_tag_init(LhVbrTag * v, const LhConfig * c);
void    lh_tag_add_frame(LhVbrTag * v, int kbps);
int     lh_tag_kbps(int version, int bitrate_index);
void    lh_tag_crc(LhVbrTag * v, const unsigned char *buf, long n);
int     lh_tag_placeholder(const LhVbrTag * v, const LhConfig * c, unsigned char *buf);
int     lh_tag_frame(const LhVbrTag * v, const LhConfig * c, int vbr_q, int enc_padding, int last_mode_ext,
                     unsigned char *buf, long size);
/* lh_tag_frame's first half -- the frame as far as the settings decide it, total_frame_size bytes -- and what the tag
 * kernel of a device-packed batch (lh_tag.hip) needs besides it; the second half is lh_tag.h's, host and device */
void    lh_tag_template(const LhVbrTag * v, const LhConfig * c, int vbr_q, unsigned char *buf);
void    lh_tag_params(const LhVbrTag * v, const LhConfig * c, LhTagParams * p);
/* ... and what the tag kernel of an incremental batch needs on top: the advance matrices by powers of two */
void    lh_tag_pow_table(LhTagPow * t);
int     lh_end_padding(long nsamples);
int     lh_end_padding_fs(long nsamples, int samples_per_frame);

/* ---- sample rate conversion in front of the encoder (lh_resample.c; reference util.c:483-697) ---- */
#define LH_RS_MAXPHASES 320     /* BPC, reference util.h */
typedef struct LhResampler {
    int     rate_in, rate_out;
    double  ratio;               /* input samples per output sample */
    int     phases, taps;
    double  clock[2];            /* input time of the next block's first sample, per channel */
    float   history[2][34];      /* the last taps + 1 input samples of the previous blocks */
    float   bank[2 * LH_RS_MAXPHASES + 1][34];
} LhResampler;

int     lh_rs_needed(int rate_in, int rate_out);
void    lh_rs_init(LhResampler * r, int rate_in, int rate_out);
int     lh_rs_block(LhResampler * r, int ch, float *out, int want, const float *in, int len, int *used);

/* A whole stream the way a batch converts it (lh_resample.c): the float planes (malloc'ed; lh_rs_free), the
 * converted length, the frame count and the end padding.  fs / mfn: samples per frame and the samples that
 * have to be buffered before a frame can be encoded. */
int     lh_rs_convert_stream(LhResampler * r, int rate_in, int rate_out, int fs, int mfn, int channels, float pcm_scale,
                             float pcm_mix, float pcm_scale_r, const short *l, const short *rr, long n, float **out_l,
                             float **out_r, long *conv_len, int *frames, int *padding);
void    lh_rs_free(void *p);

/* The same conversion as a plan: the blocks it consists of, without looking at a sample.  The blocks of a
 * stream's full chunks (fs input samples each) are those of every stream with as many chunks -- the trunk,
 * kept once and grown on demand --; its last partial chunk and the flush are the stream's own tail. */
typedef struct LhRsCursor {
    double  clock;
    long long in_at;            /* input samples consumed */
    long long fed;              /* output samples made */
    long    mf_size;
    int     frames;
    int     nblk;               /* blocks so far */
} LhRsCursor;

typedef struct LhRsTrunk {
    int     fs, mfn;
    long    nchunks;            /* chunks planned: after[0 .. nchunks] are valid */
    long    cap_chunks;
    LhRsCursor *after;          /* after[c]: the converter behind c full chunks; after[c].nblk trunk blocks lead there */
    LhRsBlock *blk;
    long    cap_blk;
} LhRsTrunk;

void    lh_rs_trunk_init(LhRsTrunk * t, int fs, int mfn);
void    lh_rs_trunk_free(LhRsTrunk * t);
int     lh_rs_trunk_extend(const LhResampler * r, LhRsTrunk * t, long nchunks);
/* the tail of a stream of n input samples behind trunk block after[n / fs].nblk (the trunk must reach that far);
 * returns the number of tail blocks -- only the first `cap' are written -- or -1 */
int     lh_rs_plan_tail(const LhResampler * r, const LhRsTrunk * t, long n, LhRsBlock * tail, int cap, long *conv_len,
                        int *frames, int *padding);
/* trunk prefix and tail of one stream in one list (at most `cap' written); *ntrunk = length of the prefix */
int     lh_rs_plan(const LhResampler * r, int fs, int mfn, long n, LhRsBlock * out, int cap, int *ntrunk, long *conv_len,
                   int *frames, int *padding);
/* The plan of a stream fed call by call (an incremental batch), from a cursor of its own: lh_rs_cursor_init is the
 * converter before its first sample (what the trunk's after[0] holds).
 * lh_rs_plan_call: one lame_encode_buffer call of m input samples at the cursor -- blocks of want = fs and len = what is
 * left of the call until the call is used up --; the cursor advances past the call.
 * lh_rs_plan_flush: the flush from the cursor -- the frames still owed, fed with bunches of zeros --; *padding is the
 * end padding, the cursor ends at the stream's converted length and frame count.
 * Both return the number of blocks and write only the first `cap' (blk == NULL: none). */
void    lh_rs_cursor_init(LhRsCursor * c);
int     lh_rs_plan_call(const LhResampler * r, int fs, int mfn, LhRsCursor * c, int m, LhRsBlock * blk, int cap);
int     lh_rs_plan_flush(const LhResampler * r, int fs, int mfn, LhRsCursor * c, LhRsBlock * blk, int cap, int *padding);
/* the tiles of one block, in output order: each as many outputs as touch at most LH_RS_SPAN_MAX input positions, measured
 * with lh_rs_locate; none for a block that makes nothing.  Returns their number, only the first `cap' are written */
int     lh_rs_block_tiles(const LhResampler * r, const LhRsBlock * b, int stream, LhRsTile * tiles, int cap);
/* ... with the tiles' rate class written into them (lh_rs_block_tiles: class 0) */
int     lh_rs_block_tiles_class(const LhResampler * r, const LhRsBlock * b, int stream, int cls, LhRsTile * tiles, int cap);
/* The pass-through plan: a stream whose rate the reference does not convert (lh_rs_needed == 0) gets a converter without
 * a bank, with which lh_rs_plan_call / _flush cut the blocks fill_buffer cuts -- made = used = min(frame size, samples
 * at hand) -- and the flush owes nothing for a converter's delay; lh_rs_block_tiles gives every such block one tile. */
void    lh_rs_init_identity(LhResampler * r, int rate_in, int rate_out);
int     lh_rs_is_identity(const LhResampler * r);
/* one block of a plan evaluated on the host, sample by sample as the device kernel does it: writes
 * out_l / out_r [out_at, out_at + made) */
void    lh_rs_eval_block(const LhResampler * r, const LhRsBlock * b, int channels, float pcm_scale, float pcm_mix,
                         float pcm_scale_r, const short *l, const short *rr, long n, float *out_l, float *out_r);

/* ---- ReplayGain "radio gain" for the LAME tag (lh_replaygain.c; reference gain_analysis.c) ---- */
#define LH_RG_BINS 12000        /* 0.01 dB steps up to 120 dB */
#define LH_RG_MAX_BLOCK 2404    /* a piece never exceeds a 50 ms window at 48 kHz */
typedef struct LhReplayGain {
    int     rate_index;          /* row of the filter tables; -1 = off */
    long    window, filled;      /* samples per 50 ms window / in the current one */
    double  lsum, rsum;          /* the window's energies so far */
    float   hist_in[2][10], hist_mid[2][10], hist_out[2][10];   /* the last ten samples before / between / after the filters */
    uint32_t bins[LH_RG_BINS];
    float   work[3][10 + LH_RG_MAX_BLOCK];
} LhReplayGain;

int     lh_rg_start(LhReplayGain * g, int samplerate);
int     lh_rg_block(LhReplayGain * g, const float *l, const float *r, int n, int channels);
int     lh_rg_finish(LhReplayGain * g);
/* what lh_rg_block / lh_rg_finish make of a window's sums and of the histogram: one text for the handle's host analysis
 * and for the window sums a batch's device analysis brings back */
size_t  lh_rg_bin(double lsum, double rsum, long window);
int     lh_rg_tenths(const uint32_t * bins);
int     lh_gain_from_windows(const double *pairs, long nwin, long window);
/* a batch stream's analysis as a plan -- the blocks lame_encode_buffer would hand to lh_rg_block, from the stream's length
 * alone; rs == NULL: no rate conversion -- and the plan evaluated on host samples (lh_gain.hip's twin) */
int     lh_gain_plan(const LhResampler * rs, int fs, int mfn, long n, int *blocks, int cap, long *total);
/* the same for a stream fed call by call (an incremental batch without rate conversion): a cursor per stream -- samples the
 * analysis has heard, and the samples fed / frames out as lame_encode_flush counts them --, one call of m samples, the flush */
typedef struct LhGainCursor {
    long long heard;
    long long fed;
    long    frames;
} LhGainCursor;
void    lh_gain_cursor_init(LhGainCursor * c);
int     lh_gain_plan_call(LhGainCursor * c, int fs, int mfn, int m, int *blocks, int cap);
int     lh_gain_plan_flush(LhGainCursor * c, int fs, int mfn, int *blocks, int cap);
long    lh_gain_eval_host(int samplerate, int channels, const int *blocks, int nblocks, const float *l, const float *r, long n,
                          double *pairs, long cap, int *tenths);

#ifdef __cplusplus
}
#endif
#endif
