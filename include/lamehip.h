/*
 * lamehip.h -- C ABI of liblamehip: the MI355X-native MP3 encode inner loop
 * behind the reference's public API.
 *
 * Part 1 mirrors the subset of the reference's include/lame.h that its frontend
 * uses for CBR encoding; each entry point cites the reference declaration it
 * replaces (file:line under /root/reference).  Names, argument meaning, return
 * codes and the output lag (first call returns 0 bytes) are the reference's.
 * Part 2 is the batch extension the GPU needs: a single lame_encode_buffer call
 * carries 26 ms of one stream, a batch call carries whole streams for thousands
 * of handles.
 *
 * Everything here is plain C: pointers and sizes only, no torch / HIP types.
 * Unsupported settings (free format) make
 * lame_init_params() return -1 instead of silently taking another path, and
 * every call fails with LAMEHIP_ERR_NODEVICE when no HIP device is present --
 * there is no CPU fallback inside this library.
 */
#ifndef LAMEHIP_H
#define LAMEHIP_H

#include <stdint.h>
#include <stddef.h>
#include <stdarg.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAMEHIP_ERR_NODEVICE (-10)
#define LAMEHIP_ERR_DEVICE   (-11)     /* a HIP call failed; see lamehip_last_error() */
#define LAMEHIP_ERR_PAYLOAD  (-12)     /* device payload failed the packer's consistency checks */

/* ------------------------------------------------------------------ */
/* Part 1: lame.h-shaped handle API                                    */

struct lame_global_struct;
typedef struct lame_global_struct lame_global_flags;
typedef lame_global_flags *lame_t;

/* MPEG_mode, reference include/lame.h:61-69 */
typedef enum MPEG_mode_e { STEREO = 0, JOINT_STEREO, DUAL_CHANNEL, MONO, NOT_SET, MAX_INDICATOR } MPEG_mode;
/* vbr_mode, reference include/lame.h:49-58 */
typedef enum vbr_mode_e { vbr_off = 0, vbr_mt, vbr_rh, vbr_abr, vbr_mtrh, vbr_max_indicator,
    vbr_default = vbr_mtrh } vbr_mode;

lame_t  lame_init(void);                                            /* lame.h:168 */
int     lame_set_in_samplerate(lame_t, int);                         /* lame.h:188 */
int     lame_get_in_samplerate(const lame_t);                        /* lame.h:189 */
int     lame_set_num_channels(lame_t, int);                          /* lame.h:192 (2, or 1 = mono: only buffer_l is read) */
int     lame_get_num_channels(const lame_t);                         /* lame.h:193 */
int     lame_set_out_samplerate(lame_t, int);                        /* lame.h:224 (0 = by bitrate; != input rate: converted) */
int     lame_get_out_samplerate(const lame_t);                       /* lame.h:225 */
int     lame_set_brate(lame_t, int);                                 /* lame.h:353 */
int     lame_get_brate(const lame_t);                                /* lame.h:354 */
int     lame_set_mode(lame_t, MPEG_mode);                            /* lame.h:270 */
MPEG_mode lame_get_mode(const lame_t);                               /* lame.h:271 */
int     lame_set_quality(lame_t, int);                               /* lame.h:263 */
int     lame_get_quality(const lame_t);                              /* lame.h:264 */
int     lame_set_VBR(lame_t, vbr_mode);                              /* lame.h:432 (vbr_off, vbr_abr, vbr_mt / vbr_mtrh) */
vbr_mode lame_get_VBR(const lame_t);                                 /* lame.h:433 */
int     lame_set_VBR_q(lame_t, int);                                 /* lame.h:436 (0 best .. 9; default 4) */
int     lame_get_VBR_q(const lame_t);                                /* lame.h:437 */
int     lame_set_preset(lame_t, int);                     /* --preset: V0..V9, named presets, 8..320 = ABR; lame.h:359 */
int     lame_set_VBR_quality(lame_t, float);              /* -V n.f, lame.h:393 */
float   lame_get_VBR_quality(const lame_t);
int     lame_set_VBR_min_bitrate_kbps(lame_t, int);       /* -b with VBR / ABR, lame.h:403 */
int     lame_get_VBR_min_bitrate_kbps(const lame_t);
int     lame_set_VBR_max_bitrate_kbps(lame_t, int);       /* -B, lame.h:406 */
int     lame_get_VBR_max_bitrate_kbps(const lame_t);
int     lame_set_VBR_hard_min(lame_t, int);               /* -F: the minimum also holds for digital silence, lame.h:413 */
int     lame_get_VBR_hard_min(const lame_t);
int     lame_set_VBR_mean_bitrate_kbps(lame_t, int);                 /* lame.h:444 (ABR mean, with lame_set_VBR(vbr_abr)) */
int     lame_get_VBR_mean_bitrate_kbps(const lame_t);                /* lame.h:445 */
int     lame_set_bWriteVbrTag(lame_t, int);                          /* lame.h:240 (default 1, as in the reference) */
int     lame_get_bWriteVbrTag(const lame_t);                         /* lame.h:241 */
int     lame_set_findReplayGain(lame_t, int);                        /* lame.h:296 (accepted, ignored) */
/* frontend switches (-m f, --nores, -p, -c, -o, -e, --strictly-enforce-ISO, --lowpass, --scale*,
 * --noshort, --shortblocks); values and defaults are the reference's */
int     lame_set_force_ms(lame_t, int);                              /* lame.h:288 (joint stereo only) */
int     lame_get_force_ms(const lame_t);
int     lame_set_disable_reservoir(lame_t, int);                     /* lame.h:400 */
int     lame_get_disable_reservoir(const lame_t);
int     lame_set_error_protection(lame_t, int);                      /* lame.h:376 (CRC-16 after the header) */
int     lame_get_error_protection(const lame_t);
int     lame_set_copyright(lame_t, int);                             /* lame.h:368 */
int     lame_get_copyright(const lame_t);
int     lame_set_original(lame_t, int);                              /* lame.h:372 */
int     lame_get_original(const lame_t);
int     lame_set_emphasis(lame_t, int);                              /* lame.h:558 */
int     lame_get_emphasis(const lame_t);
int     lame_set_extension(lame_t, int);                             /* lame.h:387 */
int     lame_get_extension(const lame_t);
int     lame_set_strict_ISO(lame_t, int);                            /* lame.h:391 (0 default, 1 strict, 2 maximum) */
int     lame_get_strict_ISO(const lame_t);
int     lame_set_lowpassfreq(lame_t, int);                           /* lame.h:470 (Hz; 0 default, -1 none) */
int     lame_get_lowpassfreq(const lame_t);
int     lame_set_lowpasswidth(lame_t, int);                          /* lame.h:473 */
int     lame_get_lowpasswidth(const lame_t);
int     lame_set_scale(lame_t, float);                               /* lame.h:199 */
int     lame_set_scale_left(lame_t, float);                          /* lame.h:206 */
int     lame_set_scale_right(lame_t, float);                         /* lame.h:213 */
int     lame_set_allow_diff_short(lame_t, int);                      /* lame.h:535 */
int     lame_set_no_short_blocks(lame_t, int);                       /* lame.h:547 */
int     lame_set_force_short_blocks(lame_t, int);                    /* lame.h:551 */
int     lame_init_params(lame_t);                                    /* lame.h:636 */
int     lame_get_framesize(const lame_t);                            /* lame.h:582 */
int     lame_get_frameNum(const lame_t);                             /* lame.h:597 */
int     lame_get_encoder_delay(const lame_t);                        /* lame.h:571 */
int     lame_get_encoder_padding(const lame_t);                      /* lame.h:579, known after lame_encode_flush */
int     lame_get_mf_samples_to_encode(const lame_t);                 /* lame.h:585 */
int     lame_set_num_samples(lame_t, unsigned long);                 /* lame.h:184 */
unsigned long lame_get_num_samples(const lame_t);
int     lame_get_totalframes(const lame_t);                          /* lame.h:603 */
/* histograms over the frames encoded so far, for a frontend's progress display (lame.h:893-960) */
void    lame_bitrate_kbps(const lame_t, int bitrate_kbps[14]);
void    lame_bitrate_hist(const lame_t, int bitrate_count[14]);
void    lame_stereo_mode_hist(const lame_t, int stereo_mode_count[4]);
void    lame_bitrate_stereo_mode_hist(const lame_t, int bitrate_stmode_count[14][4]);
void    lame_block_type_hist(const lame_t, int btype_count[6]);
void    lame_bitrate_block_type_hist(const lame_t, int bitrate_btype_count[14][6]);
/* message callbacks (lame.h:346-348): a failed call on the handle hands its explanation -- the text
 * lamehip_last_error() returns -- to errorf; the default prints to stderr like the reference's,
 * NULL silences.  debugf / msgf are stored for the frontend's sake (this library is quiet). */
typedef void (*lame_report_function)(const char *format, va_list ap);
int     lame_set_errorf(lame_t, lame_report_function);                   /* lame.h:346 */
int     lame_set_debugf(lame_t, lame_report_function);                   /* lame.h:347 */
int     lame_set_msgf(lame_t, lame_report_function);                     /* lame.h:348 */
int     lame_get_version(const lame_t);                              /* lame.h:568 */
/* The frontend's tuning switches (its "experimental" section).  A value left alone takes the bitrate's / quality's
 * preset value or the default of lame_init_params, exactly as in the reference (presets.c SET_OPTION, lame.c:1112-1203);
 * every one only changes constants and tables that reach the kernels.  lame_set_free_format(1), lame_set_experimentalZ
 * and lame_set_ATHonly(1) are accepted here and make lame_init_params fail (not on this path). */
void    lame_set_msfix(lame_t, double);                              /* lame.h:424 */
float   lame_get_msfix(const lame_t);
int     lame_set_ATHtype(lame_t, int);                               /* lame.h:502 */
int     lame_get_ATHtype(const lame_t);
int     lame_set_ATHlower(lame_t, float);                            /* lame.h:506 */
float   lame_get_ATHlower(const lame_t);
int     lame_set_athaa_type(lame_t, int);                            /* lame.h:510 */
int     lame_get_athaa_type(const lame_t);
int     lame_set_athaa_sensitivity(lame_t, float);                   /* lame.h:521 */
float   lame_get_athaa_sensitivity(const lame_t);
int     lame_set_ATHonly(lame_t, int);                               /* lame.h:490 */
int     lame_set_ATHshort(lame_t, int);                              /* lame.h:494 */
int     lame_set_noATH(lame_t, int);                                 /* lame.h:498 */
int     lame_set_interChRatio(lame_t, float);                        /* lame.h:543 */
int     lame_set_useTemporal(lame_t, int);                           /* lame.h:539 */
int     lame_set_highpassfreq(lame_t, int);                          /* lame.h:477 */
int     lame_set_highpasswidth(lame_t, int);                         /* lame.h:480 */
int     lame_set_exp_nspsytune(lame_t, int);                         /* lame.h:421 */
int     lame_get_exp_nspsytune(const lame_t);
int     lame_set_experimentalY(lame_t, int);                         /* lame.h:413 */
int     lame_set_experimentalZ(lame_t, int);                         /* lame.h:417 */
int     lame_set_free_format(lame_t, int);                           /* lame.h:292 */
int     lame_get_free_format(const lame_t);
int     lame_set_compression_ratio(lame_t, float);                   /* lame.h:355 */
float   lame_get_compression_ratio(const lame_t);
/* ReplayGain of the input for the LAME tag (the frontend's default): measured on the host, lh_replaygain.c */
int     lame_set_findReplayGain(lame_t, int);                        /* lame.h:296 */
int     lame_get_RadioGain(const lame_t);                            /* lame.h:606 */
/* parts of the reference this library does not have (decoder, assembler variants): "off" is accepted */
int     lame_set_decode_only(lame_t, int);                           /* lame.h:244 */
int     lame_set_asm_optimizations(lame_t, int, int);                /* lame.h:360 */
int     lame_set_nogap_total(lame_t, int);                           /* lame.h:326 */
int     lame_set_nogap_currentindex(lame_t, int);                    /* lame.h:329 */
void    lame_print_config(const lame_t);                             /* lame.h:678 */
void    lame_print_internals(const lame_t);                          /* lame.h:680 */
int     lame_get_bitrate(int mpeg_version, int table_index);         /* lame.h:1290 */
int     lame_get_samplerate(int mpeg_version, int table_index);      /* lame.h:1291 */
const char *get_lame_version(void);                                  /* lame.h:644 */
const char *get_lame_short_version(void);
const char *get_lame_very_short_version(void);
const char *get_psy_version(void);
const char *get_lame_url(void);
const char *get_lame_os_bitness(void);

/* return: bytes written to mp3buf (may be 0); -1 mp3buf too small; -2 alloc;
 * -3 lame_init_params not called; mp3buf_size == 0 disables the size check
 * (reference lame.h:687-722) */
int     lame_encode_buffer(lame_t, const short int buffer_l[], const short int buffer_r[],
                           const int nsamples, unsigned char *mp3buf, const int mp3buf_size);   /* lame.h:715 */
int     lame_encode_buffer_interleaved(lame_t, short int pcm[], int num_samples,
                                       unsigned char *mp3buf, int mp3buf_size);                  /* lame.h:730 */
/* the other sample types of the reference (same return codes); each sample goes through the
 * type's scale and the pcm_transform matrix exactly as lame_copy_inbuffer does */
int     lame_encode_buffer_float(lame_t, const float l[], const float r[], const int nsamples,
                                 unsigned char *mp3buf, const int mp3buf_size);                  /* lame.h:746 (+/-32768) */
int     lame_encode_buffer_ieee_float(lame_t, const float l[], const float r[], const int nsamples,
                                      unsigned char *mp3buf, const int mp3buf_size);             /* lame.h:758 (+/-1.0) */
int     lame_encode_buffer_interleaved_ieee_float(lame_t, const float pcm[], const int nsamples,
                                                  unsigned char *mp3buf, const int mp3buf_size); /* lame.h:765 */
int     lame_encode_buffer_ieee_double(lame_t, const double l[], const double r[], const int nsamples,
                                       unsigned char *mp3buf, const int mp3buf_size);            /* lame.h:776 */
int     lame_encode_buffer_interleaved_ieee_double(lame_t, const double pcm[], const int nsamples,
                                                   unsigned char *mp3buf, const int mp3buf_size);        /* lame.h:783 */
int     lame_encode_buffer_long(lame_t, const long l[], const long r[], const int nsamples,
                                unsigned char *mp3buf, const int mp3buf_size);                   /* lame.h:799 (+/-32768) */
int     lame_encode_buffer_long2(lame_t, const long l[], const long r[], const int nsamples,
                                 unsigned char *mp3buf, const int mp3buf_size);                  /* lame.h:813 (+/-2^63) */
int     lame_encode_buffer_int(lame_t, const int l[], const int r[], const int nsamples,
                               unsigned char *mp3buf, const int mp3buf_size);                    /* lame.h:831 (+/-2^31) */
int     lame_encode_flush(lame_t, unsigned char *mp3buf, int size);                              /* lame.h:856 */
/* --nogap: end a file without draining the sample buffers, then start the next one (lame.h:870, 886) */
int     lame_encode_flush_nogap(lame_t, unsigned char *mp3buf, int size);
int     lame_init_bitstream(lame_t);
/* final Xing/Info + LAME tag frame that replaces the placeholder at the head of the stream */
size_t  lame_get_lametag_frame(const lame_t, unsigned char *buffer, size_t size);                /* lame.h:970 */
int     lame_close(lame_t);                                                                      /* lame.h:977 */

/* ------------------------------------------------------------------ */
/* Part 2: batch extension (not in lame.h)                             */

typedef struct lamehip_batch lamehip_batch;

/* B independent streams that share the settings of `proto' (which must have
 * passed lame_init_params); capacity = samples per channel per stream. */
lamehip_batch *lamehip_batch_create(const lame_t proto, int nstreams, long capacity_samples);
/* the same on HIP device `device' (0 .. lamehip_device_count() - 1) instead of the calling thread's
 * current one.  A batch keeps its device: every later call on it runs there and leaves the
 * caller's current device as it was.  This is what one host thread per GPU uses to shard a batch
 * of independent streams over the GPUs of a node (no inter-device traffic). */
lamehip_batch *lamehip_batch_create_on(int device, const lame_t proto, int nstreams, long capacity_samples);
/* device of a handle's own (per-frame) launches; before lame_init_params.  Default: the device
 * that is current when lame_init_params runs. */
int     lamehip_set_device(lame_t, int device);
void    lamehip_batch_destroy(lamehip_batch *);
/* copy one stream's planar s16 PCM host -> HBM (H2D, synchronous).  When proto's input rate differs from
 * its output rate the stream is converted exactly as the reference converts it when lame_encode_buffer is
 * fed a frame of input samples per call (util.c:520-697); capacity and lengths then count input samples.
 * By default this call converts on the host, and the _device variants, lamehip_batch_set_length and the
 * pinned mirror below are refused: lamehip_batch_set_device_resampling moves the conversion to the device
 * and opens them. */
int     lamehip_batch_set_pcm(lamehip_batch *, int stream, const short *l, const short *r, long nsamples);
/* same, from planar s16 buffers that already live in HBM (D2D) */
int     lamehip_batch_set_pcm_device(lamehip_batch *, int stream, const void *dev_l, const void *dev_r, long nsamples);
/* device pointer of the PCM pool: int16 [stream][2][capacity] -- int32 or float on a batch of another sample type
 * (lamehip_batch_set_sample_type) --; lets a producer that already lives on the GPU fill it in place (then declare
 * lengths) */
void   *lamehip_batch_pcm_device_ptr(lamehip_batch *);
int     lamehip_batch_set_length(lamehip_batch *, int stream, long nsamples);
/* Rate conversion on the device, for a batch whose input rate differs from its output rate (-1 for any other, and
 * -1 once PCM, a length or the pinned mirror has been handed over; lamehip_last_error() says which).  Switched on,
 * the batch keeps its input as s16 at the input rate in a pool [stream][2][capacity], and lamehip_batch_set_pcm,
 * _set_pcm_device, _pcm_device_ptr, _set_length, _pcm_host_ptr, _mark_pcm and _upload work as on a batch that does
 * not convert.  Declaring a length plans the conversion on the host without looking at a sample -- converted length,
 * lamehip_batch_frames and the tag's padding are known at once; -1 when the converted stream exceeds the pool --, and
 * lamehip_batch_encode converts the streams declared (lamehip_batch_set_pcm* / _set_length / _mark_pcm) since their
 * last conversion with a kernel on the batch's stream, in front of the analysis kernels.  Samples at or beyond a
 * stream's length are never read.  Same floats, hence same bytes, as the host conversion.  An allocation failure
 * returns LAMEHIP_ERR_DEVICE and leaves the batch as it was.  lamehip_batch_append and the other incremental calls
 * stay refused on a converting batch unless lamehip_batch_set_incremental_resampling (below) opens them. */
int     lamehip_batch_set_device_resampling(lamehip_batch *, int on);
/* Incremental use of a batch that converts the rate on the device: a live producer at one rate, the encoder at another.
 * Accepted only with lamehip_batch_set_device_resampling on (-1 otherwise, lamehip_last_error() names that call) and only
 * before any PCM, length or mirror has been handed over; before or after lamehip_batch_set_sample_type.  With it on,
 * lamehip_batch_append (an s16 batch), lamehip_batch_append_input, _append_input_device and _append_device take chunks
 * at the INPUT rate in the batch's element type: every call is one call of the reference entry point the type is named
 * after, converter included -- the reference cuts a call into blocks of at most one frame of output and carries its
 * clock and filter tail from call to call, so the bytes depend on how the stream is cut into calls, and
 * lamehip_batch_drain hands over the bytes that call would have returned.  The chunks land in the input pool as they
 * are; lamehip_batch_encode_available and lamehip_batch_finish convert what was appended since the last round with ONE
 * kernel launch (lamehip_batch_last_resample_ms: that launch) in front of the encode launch, lamehip_batch_finish also
 * the flush.  Capacity counts input samples; an append is also refused (-1, nothing counted) when its stream, flushed
 * right after the call, would exceed the float pool -- lamehip_batch_finish therefore never lacks room.  Device packing
 * stays refused on an incremental batch unless lamehip_batch_set_incremental_packing, ReplayGain is refused unless
 * lamehip_batch_set_incremental_replaygain.  Until the first append the batch takes whole streams as before.
 * An allocation failure returns LAMEHIP_ERR_DEVICE and leaves the batch as it was. */
int     lamehip_batch_set_incremental_resampling(lamehip_batch *, int on);
/* Every stream at its own input rate: a pool of slots fed at 8, 16, 22.05, 32, 44.1, 48, 96 kHz ... that all come out as the
 * batch's one kind of MP3.  lamehip_batch_set_stream_in_samplerate tells a batch that converts round by round (both switches
 * above on) that stream s arrives at hz.  From then on the stream's bytes, frames, end padding, tag frame
 * (lamehip_batch_set_incremental_tagging: the info byte's source-frequency and "non-optimal" bits are the stream's) and
 * radio gain are those of a reference handle with the batch's settings, lame_set_in_samplerate(hz) and
 * lame_set_out_samplerate(R) given explicitly, R the batch's resolved output rate, fed the same calls -- each append one
 * lame_encode_buffer* call, as on any such batch.  A rate the reference does not convert (within +-0.05 % of R:
 * 44 077 .. 44 122 Hz for 44.1 kHz) is not converted here either: the samples pass the PCM matrix only.
 *   accepted rates   any hz > 0 for which the library's host init resolves the batch's configuration and tables again with
 *                    (in = hz, out = R explicit, every other setting the handle's); the resolved records are compared, and
 *                    -1 names the record and the byte that differs
 *   when             the stream has nothing appended yet: a fresh batch, after lamehip_batch_reset, after
 *                    lamehip_batch_restart_stream and before the first append; -1 otherwise.  lamehip_batch_reset and
 *                    lamehip_batch_restart_stream put a stream back at the batch's own rate: a slot's next tenant states
 *                    its rate again
 *   capacity         still counts input samples per stream at whatever rate; the float pool's rows stay what the batch's own
 *                    rate gives them, so a stream at a lower rate fills its row sooner, and the appends' refusal ("flushed
 *                    behind this call, would be ... converted samples") is computed with the stream's own converter
 *   classes          distinct rates alive in a batch are classes, 16 at most, the batch's own rate one of them; a class -- its
 *                    converter and its bank of kernels in HBM -- is made on first use and lives until lamehip_batch_destroy;
 *                    one more is refused (-1); an allocation failure returns LAMEHIP_ERR_DEVICE and leaves the batch as it
 *                    was
 *   refused (-1, lamehip_last_error() names the call)   a batch without lamehip_batch_set_incremental_resampling, a finished
 *                    batch, no such stream, hz <= 0, a stream that has samples or has ended -- and, once any stream has a
 *                    rate other than the batch's, lamehip_batch_set_pcm*, _set_input*, _set_length and lamehip_batch_encode:
 *                    the one-shot converter shares one trunk of blocks between all streams and stays single-rate
 * A round with such a stream converts all rates in ONE launch (csrc/lh_resample_dev.hip: lh_resample_mixed_tiles_kernel,
 * timed by lamehip_batch_last_resample_ms as before); a batch that never makes the call gets the launches, kernels, layouts
 * and bytes it always got.  lamehip_batch_stream_in_samplerate returns the stream's rate, the batch's own when none was
 * set; -1: no such stream. */
int     lamehip_batch_set_stream_in_samplerate(lamehip_batch *, int stream, int hz);
int     lamehip_batch_stream_in_samplerate(lamehip_batch *, int stream);
/* test accessor: the converted signal of a stream (float planes as the encoder reads them), valid after
 * lamehip_batch_set_pcm when the host converts and after lamehip_batch_encode when the device does -- also the float
 * planes of a batch of another sample type that does not convert, after lamehip_batch_encode, or, on an incremental
 * batch of such a type, up to what has reached the pool (device-resident appends at once, staged ones with the next
 * lamehip_batch_encode_available / _finish), and on an incremental batch that converts, what the rounds so far have
 * converted --; waits for the batch's stream.  Returns the converted length, or a negative code (-1 also when it exceeds cap). */
long    lamehip_batch_get_converted(lamehip_batch *, int stream, float *l, float *r, long cap);
/* HIP-event time in ms of the device conversion of the last lamehip_batch_encode (after lamehip_batch_sync), or of the
 * last lamehip_batch_encode_available / _finish of an incremental batch that converts; 0 when none ran.  It is not part
 * of lamehip_batch_last_kernel_ms / _parts_ms. */
float   lamehip_batch_last_resample_ms(lamehip_batch *);

/* Sample types of a batch's input, each named after the reference entry point whose bytes it reproduces (lame.c:1786-1972:
 * lame_encode_buffer_template with the type's norm, lame_copy_inbuffer's arithmetic in float): */
#define LAMEHIP_PCM_S16      0  /* int16_t, +/- 32768: lame_encode_buffer (the default) */
#define LAMEHIP_PCM_S32      1  /* int32_t, +/- 2^31:  lame_encode_buffer_int */
#define LAMEHIP_PCM_F32      2  /* float,   +/- 32768: lame_encode_buffer_float */
#define LAMEHIP_PCM_F32_UNIT 3  /* float,   +/- 1.0:   lame_encode_buffer_ieee_float */
/* The batch's sample type.  Only before any PCM, length or mirror has been handed over (-1 after, and lamehip_last_error()
 * says so).  With a type other than s16 the batch holds an input pool T [stream][2][capacity] of that element type (pinned
 * mirror, device pointer, lamehip_batch_set_length, _mark_pcm and _upload work on it as on the s16 pool) and a float pool
 * [stream][2][capacity] that the kernels read: 8 bytes per sample and plane in HBM against 2.  lamehip_batch_encode fills
 * the float pool from the input pool with a kernel on the batch's stream, in front of the analysis kernels, for the streams
 * declared (lamehip_batch_set_input* / _set_length / _mark_pcm) since their last ingest; samples at or beyond a stream's
 * length are never read.  Same floats as the reference's lame_copy_inbuffer, hence the bytes of the entry point named above.
 * On a batch whose input rate differs from its output rate a type other than s16 needs
 * lamehip_batch_set_device_resampling(b, 1) first (-1 otherwise: the host converter takes s16 only); the converter then
 * reads the typed pool itself.  An allocation failure returns LAMEHIP_ERR_DEVICE and leaves the batch as it was.
 * lamehip_batch_append, lamehip_batch_set_pcm and lamehip_batch_set_pcm_device (the calls that take shorts) are refused on a
 * batch of another type, and lamehip_batch_pcm_host_ptr returns NULL. */
int     lamehip_batch_set_sample_type(lamehip_batch *, int type);
/* one stream's samples, of the batch's element type, from host buffers: l and r advance by `stride' elements per sample --
 * 1: planar; 2: interleaved with r = l + 1, as lame_encode_buffer_interleaved* is called.  Through the pinned mirror where
 * there is one, like lamehip_batch_set_pcm; mono without a downmix reads l only.  Works on an s16 batch too. */
int     lamehip_batch_set_input(lamehip_batch *, int stream, const void *l, const void *r, int stride, long nsamples);
/* the same from buffers in HBM, synchronous like lamehip_batch_set_pcm_device: two device-to-device copies for stride 1, a
 * small kernel that takes the interleaved buffer apart for stride 2.  Whatever produced the buffers must have finished. */
int     lamehip_batch_set_input_device(lamehip_batch *, int stream, const void *dev_l, const void *dev_r, int stride, long nsamples);
/* the pinned mirror of the input pool in the batch's element type, [stream][2][capacity] (lamehip_batch_pcm_host_ptr for
 * any type; the same rules: ask again before rewriting rows an asynchronous upload has taken) */
void   *lamehip_batch_input_host_ptr(lamehip_batch *);
/* HIP-event time in ms of the ingest kernel of the last lamehip_batch_encode (after lamehip_batch_sync); 0 when none ran.
 * Like lamehip_batch_last_resample_ms it is not part of lamehip_batch_last_kernel_ms / _parts_ms. */
float   lamehip_batch_last_ingest_ms(lamehip_batch *);

/* ReplayGain of a batch: with the switch on, lamehip_batch_encode measures every stream's radio gain on the device (one
 * kernel on the batch's stream, behind the conversion / ingest and in front of the analysis kernels, once per call) for
 * the streams declared since their last analysis, and lamehip_batch_pack_tagged / _get_bytes_tagged write it into the LAME
 * tag.  Stream s gets the value lame_get_RadioGain returns on the handle API after lame_encode_flush for the same settings
 * and the same samples handed over a frame's worth (1152, MPEG-2 / 2.5: 576 input samples) per lame_encode_buffer call
 * with lame_set_findReplayGain(1).  Call it before lamehip_batch_encode.  The proto's lame_set_findReplayGain is not
 * inherited.  -1 on an incremental batch, and once it is on lamehip_batch_append / _encode_available / _finish return -1
 * (lamehip_last_error) unless lamehip_batch_set_incremental_replaygain (below) opened them; LAMEHIP_ERR_DEVICE when an allocation fails, the batch is then as it was.
 * The window sums of a launch stay on the device until a getter or a tagged output asks for them; a lamehip_batch_encode
 * that finds those of the launch before it still there fetches them first, and for that WAITS for the batch's stream on the
 * host.  A caller that pipelines rounds reads the gains of a round (lamehip_batch_radio_gain, after lamehip_batch_sync or
 * the fetch) before it encodes the next. */
int     lamehip_batch_set_replaygain(lamehip_batch *, int on);
/* ReplayGain of an incremental batch, carried round by round on the device.  Accepted only before any PCM, length, mirror or
 * append has been handed over (-1 after, lamehip_last_error() names this call); before or after
 * lamehip_batch_set_sample_type; on a batch that converts the rate only with lamehip_batch_set_incremental_resampling on
 * already (-1, the error names that call); on a batch that packs on the device only with
 * lamehip_batch_set_incremental_packing on already (-1 otherwise).  on = 0 before the first append
 * puts the batch back as it was; an allocation failure returns LAMEHIP_ERR_DEVICE and leaves the batch as it was.
 * With it on, lamehip_batch_append, _append_input, _append_input_device and _append_device are accepted: each is one call of
 * the reference entry point the batch's sample type is named after, made with lame_set_findReplayGain(1) -- the reference
 * hands its analysis a call's samples in blocks of at most one frame counted from the call's start (a converting batch: the
 * blocks the converter makes), and the analysis cuts its sums at a block's start, so the window sums depend on how the stream
 * is cut into calls.  lamehip_batch_encode_available and lamehip_batch_finish run ONE launch of the gain kernel over what was
 * appended since the last round (lamehip_batch_finish: the flush as well), behind the append and conversion launches, on the
 * batch's stream and timed by events of its own (lamehip_batch_last_gain_ms: that launch; not part of
 * lamehip_batch_last_kernel_ms).  Filter histories, the open window's sums and the samples heard stay in HBM between rounds;
 * a round that brings a stream nothing leaves its state untouched.  lamehip_batch_get_gain_windows returns the windows
 * finished so far after any round (they come home with the round's wait); lamehip_batch_radio_gain is valid after
 * lamehip_batch_finish -- what lame_get_RadioGain returns on the handle API after lame_encode_flush for the same settings and
 * the same sequence of calls -- and -1 before (the error names lamehip_batch_finish: the handle has no value before its flush
 * either).  lamehip_batch_reset clears carried state, windows and gains.  An append whose stream, flushed right after the
 * call, would be longer than the analysis takes (0x7fffff00 samples) is refused: -1, nothing counted, the error names the
 * call.  Until the first append the batch behaves as one with lamehip_batch_set_replaygain(b, 1): whole streams through
 * lamehip_batch_encode.  An incremental batch writes the gain into a tag only through lamehip_batch_set_incremental_tagging:
 * lamehip_batch_tag_ptr / _get_tags_all put it into the frame they hand out. */
int     lamehip_batch_set_incremental_replaygain(lamehip_batch *, int on);
/* stream's radio gain in tenths of a dB (0 when not one 50 ms window was completed); waits for the batch's stream.  -1
 * before a lamehip_batch_encode with the switch on, and again after lamehip_batch_reset; on an incremental batch -1 before
 * lamehip_batch_finish -- or, for a stream ended on its own, before the round behind its lamehip_batch_end_stream. */
int     lamehip_batch_radio_gain(lamehip_batch *, int stream, int *tenths_db);
/* test accessor: what the kernel measured, (left sum, right sum) of the squares of every completed window; writes the first
 * cap_windows pairs and returns the number of windows, or a negative code (an incremental batch: the windows finished so far) */
long    lamehip_batch_get_gain_windows(lamehip_batch *, int stream, double *lr_pairs, long cap_windows);
/* HIP-event time in ms of the gain kernel of the last lamehip_batch_encode (after lamehip_batch_sync), or of the last
 * lamehip_batch_encode_available / _finish of a batch that measures round by round; 0 when none ran.  Like
 * lamehip_batch_last_resample_ms it is not part of lamehip_batch_last_kernel_ms / _parts_ms.  (The kernel has two mappings
 * of its serial part with the same results; the number of streams in a launch picks the faster, environment
 * LAMEHIP_GAIN_LANES=0 / 1 forces one: measurement, tests.) */
float   lamehip_batch_last_gain_ms(lamehip_batch *);

/* Incremental use -- lame_encode_buffer (lame.h:715-722, lame.c:1672-1775) for all streams of a batch at once:
 *   lamehip_batch_append            stage n more samples of one stream (host, pinned memory; any n >= 0, ragged
 *                                   across streams; several calls per stream may precede one encode)
 *   lamehip_batch_encode_available  ONE asynchronous H2D copy of everything staged, ONE launch that encodes
 *                                   every stream's newly complete frames, packing; returns the frame count
 *   lamehip_batch_drain             the bytes a stream has produced since its last drain: what the
 *                                   reference's lame_encode_buffer returns for the same calls (the output
 *                                   lags the input by the priming: the first 1152 samples yield 0 bytes)
 *   lamehip_batch_finish            lame_encode_flush (lame.h:869, lame.c:2041-2175) for every stream that has not
 *                                   ended on its own (lamehip_batch_end_stream, below); closes the batch
 * The first append switches the batch to this mode (its capacity still bounds a stream's total length).
 * Return codes as lame_encode_buffer's: >= 0, -1 a buffer or the capacity is too small, -2 allocation. */
int     lamehip_batch_append(lamehip_batch *, int stream, const short *l, const short *r, int nsamples);
int     lamehip_batch_encode_available(lamehip_batch *);
int     lamehip_batch_drain(lamehip_batch *, int stream, unsigned char *out, int out_size);
int     lamehip_batch_finish(lamehip_batch *);
/* Appends in the batch's own element type (lamehip_batch_set_sample_type; an s16 batch too), from host memory or from
 * HBM.  On an int32 / float batch a chunk goes through lame_copy_inbuffer's arithmetic straight into the float pool the
 * kernels read (one kernel, csrc/lh_ingest.hip: lh_append_kernel): each call is the reference entry point the type is
 * named after, and lamehip_batch_drain hands over the bytes that call would have returned.  On an s16 batch it is
 * lame_encode_buffer or, with stride 2, lame_encode_buffer_interleaved, and may be mixed with lamehip_batch_append.
 * The first call switches the batch to incremental use whatever its sample type; capacity, lamehip_batch_finish /
 * lamehip_batch_reset and lamehip_batch_drain are as above.  lamehip_batch_append (shorts) stays refused on a batch of
 * another type.  -1, with a lamehip_last_error() that names the call: a stream that would exceed the capacity, a stride
 * other than 1 or 2, a finished batch, a stream that lamehip_batch_end_stream has ended (until
 * lamehip_batch_restart_stream; lamehip_batch_append likewise), a batch that converts the sample rate without
 * lamehip_batch_set_incremental_resampling (with it the chunks are at the input rate and go to the input pool as they
 * are, see there), a batch that packs on the device -- refused unless lamehip_batch_set_incremental_packing -- or measures
 * ReplayGain -- refused unless lamehip_batch_set_incremental_replaygain, which has the gain plan follow the calls chunk by
 * chunk.
 * LAMEHIP_ERR_DEVICE when an allocation fails, the batch is then as it was.
 *   lamehip_batch_append_input         host buffers, l and r `stride' elements from sample to sample as for
 *                                      lamehip_batch_set_input; staged in the pinned arena like the shorts of
 *                                      lamehip_batch_append (16 MB: 4-byte elements halve the samples it holds), on their
 *                                      way to HBM with the next lamehip_batch_encode_available / _finish: one copy of the
 *                                      table, one of the bytes in use, one launch
 *   lamehip_batch_append_input_device  the same from buffers in HBM, synchronous like lamehip_batch_set_input_device:
 *                                      whatever produced the buffers must have finished, the call makes one launch on the
 *                                      batch's stream and returns once the samples are in the pool -- the caller may reuse
 *                                      the buffers at once
 *   lamehip_batch_append_device        one round for ALL streams from one device array, such as a producer's
 *                                      [B, C, T_chunk] tensor: stream s takes nsamples[s] samples (ragged, 0 allowed), the
 *                                      left ones from element s * stream_stride of `dev' on, the right ones plane_stride
 *                                      elements further on; ONE launch for the whole batch, synchronous as above
 * A chunk's place in its stream is fixed when it is appended, so staged and device-resident appends of one stream may
 * follow each other in any order. */
int     lamehip_batch_append_input(lamehip_batch *, int stream, const void *l, const void *r, int stride, int nsamples);
int     lamehip_batch_append_input_device(lamehip_batch *, int stream, const void *dev_l, const void *dev_r, int stride, int nsamples);
int     lamehip_batch_append_device(lamehip_batch *, const void *dev, long long stream_stride, long long plane_stride, int stride,
                                    const int *nsamples);
/* HIP-event time in ms of the append launches since, and including, the last lamehip_batch_encode_available / _finish; not
 * part of lamehip_batch_last_kernel_ms / _parts_ms, like lamehip_batch_last_ingest_ms */
float   lamehip_batch_last_append_ms(lamehip_batch *);
/* Incremental use on the device bit packer.  Accepted only with lamehip_batch_set_device_packing on (-1 otherwise,
 * lamehip_last_error() names that call), only before any PCM, length, mirror or append has been handed over, and not with
 * lamehip_batch_set_device_tagging on (device tagging puts the tag frame in front of a whole stream's bytes and is refused
 * behind it likewise; an incremental batch gets its tag frames from lamehip_batch_set_incremental_tagging).  on = 0 before the first append puts the batch back as it was: a device-packed batch that refuses every
 * append.  An allocation failure returns LAMEHIP_ERR_DEVICE and leaves the batch as it was.  With it on,
 * lamehip_batch_append, _append_input, _append_input_device and _append_device are accepted, and
 * lamehip_batch_set_incremental_resampling / _set_incremental_replaygain may be switched on behind it (both run in front of
 * the encode launch, whichever packer follows).
 * Every stream gets a fixed slice of the byte pool in HBM, laid out at the first append for a stream as long as the batch's
 * capacity (the converted capacity when the batch converts) at the largest frame the settings allow; the encode kernel's
 * packer writes there at absolute positions, round after round, and its state stays in HBM.  A round
 * (lamehip_batch_encode_available / _finish) is then the append / conversion / gain launches, the encode launch -- in
 * windows or on the fused kernel as any incremental round -- and three small launches of csrc/lh_drain.hip: no LhFrameOut
 * record comes home and no host packer runs.  The drain kernels find, per stream, the position P up to which the slice is
 * what lame_encode_buffer would have returned: the packer's cursor -- or, when a frame's main data ended exactly on the
 * start of a header that is already queued, that header's start: the reference writes a header only with the next bit
 * behind it, the device packer steps over it at once (digital silence does this frame after frame) --, and after
 * lamehip_batch_finish the end of the last frame.  They gather [drained, P) of every slice into one round buffer, every
 * stream on a 16-byte boundary; a table (offset, count, status) per stream comes home first, then ONE copy of exactly the
 * round's bytes into pinned memory, then the round's wait.  A stream the caller has not drained is gathered again with the
 * next round: the pinned buffer always holds everything undrained.  A stream whose packer reports a status makes the round
 * return LAMEHIP_ERR_PAYLOAD (lamehip_last_error() names the stream).  lamehip_batch_reset starts the batch over.
 * Off (the default): launches, layouts and bytes of every path are what they were. */
int     lamehip_batch_set_incremental_packing(lamehip_batch *, int on);
/* the bytes lamehip_batch_drain would copy, in place: on a batch with lamehip_batch_set_incremental_packing in the round's
 * pinned buffer, else in a buffer of the batch's.  Valid until the next lamehip_batch_encode_available, _finish or _reset
 * (host packer: or the stream's next _drain_ptr).  Returns their number (0: nothing new, *bytes NULL) or -1; counts as a
 * drain. */
long    lamehip_batch_drain_ptr(lamehip_batch *, int stream, const unsigned char **bytes);
/* HIP-event time in ms of the drain kernels of the last lamehip_batch_encode_available / _finish of a batch with
 * lamehip_batch_set_incremental_packing; 0 when none ran.  Not part of lamehip_batch_last_kernel_ms / _parts_ms. */
float   lamehip_batch_last_drain_ms(lamehip_batch *);
/* Streams that come and go: an incremental batch as a pool of slots.  A stream ends alone, with the next round, while the
 * others go on; its file is complete at once; its slot takes the next stream.  A batch that never makes these calls gets
 * the launches and the bytes it always got.
 *   lamehip_batch_end_stream      lame_encode_flush for ONE stream, carried out by the next lamehip_batch_encode_available
 *                                 (or lamehip_batch_finish): the call launches nothing, a round stays one encode launch for
 *                                 the whole batch.  It switches a batch that has not been fed to incremental use, as
 *                                 lamehip_batch_finish does, and is refused where that is (a batch that converts, packs on
 *                                 the device or measures ReplayGain without its round-by-round switch).  From the call on
 *                                 appends to the stream are refused: -1, nothing counted, lamehip_last_error() names
 *                                 lamehip_batch_restart_stream.  The next round encodes the stream's remaining frames with
 *                                 the reference's end padding and completes its last frame -- on a converting batch behind
 *                                 the converter's flush, on one that measures ReplayGain with the analysis' flush --, every
 *                                 other stream's newly complete frames as in any round.  Behind that round
 *                                 lamehip_batch_stream_ended returns 1, lamehip_batch_drain / _drain_ptr hand over the
 *                                 stream's last bytes, lamehip_batch_frames is its total, and lamehip_batch_tag_ptr,
 *                                 lamehip_batch_radio_gain and lamehip_batch_get_gain_windows answer for THAT stream as after
 *                                 lamehip_batch_finish (for the others the first two stay -1; lamehip_batch_get_tags_all
 *                                 reports a negative size for them).  An ended stream that is not drained is gathered again
 *                                 with every round, like any other.  -1, lamehip_last_error() names the call: a finished
 *                                 batch, a stream that is ending or has ended already, no such stream.
 *   lamehip_batch_stream_ended    1 behind the round that ended the stream, until its slot is restarted; else 0; -1 for no
 *                                 such stream
 *   lamehip_batch_restart_stream  the slot of a stream that HAS ended starts a new one: counters, packer, converter and
 *                                 analysis back in front of the first sample, windows, gain, tag frame and bytes of the old
 *                                 stream gone (pointers handed out for it are valid until this call), the slot's slice of the
 *                                 byte pool reused from its first byte; the slot's capacity bounds the new stream on its
 *                                 own.  What the slot keeps in HBM -- LhStreamState, the drain's and the tag's carry, the
 *                                 analysis' -- is put back by ONE launch (csrc/lh_slots.hip: lh_slot_restart_kernel, a
 *                                 workgroup per restarted slot) at the head of the next round, for all slots restarted since
 *                                 the last one; no neighbour's record is touched.  -1: the stream has not ended (before its
 *                                 ending round too), it has bytes that were not handed out (lamehip_last_error() names
 *                                 lamehip_batch_drain: nothing is lost silently), the batch is finished, no such stream.
 *   lamehip_batch_last_restart_ms HIP-event time in ms of that launch in front of the last round; 0 when no slot was restarted
 *                                 in the gap before it.  Not part of lamehip_batch_last_kernel_ms / _parts_ms.
 * lamehip_batch_finish flushes the streams that have not ended, leaves the others as they are and closes the batch (nothing is
 * encoded when all have ended); lamehip_batch_reset starts all slots over. */
int     lamehip_batch_end_stream(lamehip_batch *, int stream);
int     lamehip_batch_stream_ended(lamehip_batch *, int stream);     /* 1 ended, 0 not, -1 bad argument */
int     lamehip_batch_restart_stream(lamehip_batch *, int stream);
float   lamehip_batch_last_restart_ms(lamehip_batch *);

/* Statistics: what the reference keeps per stream and its frontend prints after every file (updateStats; lame_bitrate_hist,
 * lame_stereo_mode_hist, lame_bitrate_stereo_mode_hist, lame_block_type_hist, lame_bitrate_block_type_hist), for every
 * stream of a batch, counted on the device: behind every encode launch -- lamehip_batch_encode's, and every round's of an
 * incremental batch -- one small kernel (lh_stats.hip) adds the launch's frame records, where they lie in HBM, to a table of
 * 176 ints per stream.  No record comes home for it; a getter fetches the tables (704 bytes per stream) once after a launch.
 *   lamehip_batch_set_statistics  off by default; on any kind of batch (one-shot or incremental, host or device packing,
 *                                 with or without incremental packing, tagging, ReplayGain or resampling, any sample type).
 *                                 -1 once PCM, a length or an append has been handed over.  Off: nothing is allocated or
 *                                 launched.
 *   lamehip_batch_get_statistics  stream s's tables as they stand behind the last launch (the getters wait for it):
 *                                 mode[bitrate index | 15 = all][mode extension 0..3 | 4 = frames] and
 *                                 block[bitrate index | 15 = all][block type 0..3 | 4 = mixed | 5 = granules]; either may
 *                                 be null.  An incremental batch: the frames of the rounds so far, lamehip_batch_frames of
 *                                 them after lamehip_batch_finish.  lamehip_batch_encode counts from zero every time, as
 *                                 does a batch after lamehip_batch_reset; a stream that ended (lamehip_batch_end_stream)
 *                                 keeps its counts until lamehip_batch_restart_stream zeroes them, its slot's alone.
 *   lamehip_batch_get_statistics_all  every stream's: B x 176 ints, a stream's mode[16][5] then its block[16][6].
 *   lamehip_batch_bitrate_hist ... _bitrate_block_type_hist  the reference's getters with (batch, stream) in front.
 *   lamehip_batch_bitrate_kbps    the bit rates of rows 1..14 (lame_bitrate_kbps).
 *   lamehip_batch_last_stats_ms   HIP-event time in ms of the statistics launch behind the last encode launch; 0 when there
 *                                 was none.  Not part of lamehip_batch_last_kernel_ms.
 * Every getter returns 0, or -1 without the switch or for a stream the batch does not have (lamehip_last_error() names the
 * call). */
int     lamehip_batch_set_statistics(lamehip_batch *, int on);
int     lamehip_batch_get_statistics(lamehip_batch *, int stream, int mode[16][5], int block[16][6]);
int     lamehip_batch_get_statistics_all(lamehip_batch *, int *out);
int     lamehip_batch_bitrate_hist(lamehip_batch *, int stream, int bitrate_count[14]);
int     lamehip_batch_stereo_mode_hist(lamehip_batch *, int stream, int stereo_mode_count[4]);
int     lamehip_batch_bitrate_stereo_mode_hist(lamehip_batch *, int stream, int bitrate_stmode_count[14][4]);
int     lamehip_batch_block_type_hist(lamehip_batch *, int stream, int btype_count[6]);
int     lamehip_batch_bitrate_block_type_hist(lamehip_batch *, int stream, int bitrate_btype_count[14][6]);
int     lamehip_batch_bitrate_kbps(lamehip_batch *, int bitrate_kbps[14]);
float   lamehip_batch_last_stats_ms(lamehip_batch *);
/* encode every stream completely (all frames incl. the flush frames), payload
 * stays in HBM; asynchronous on the batch's HIP stream */
int     lamehip_batch_encode(lamehip_batch *);
int     lamehip_batch_sync(lamehip_batch *);
/* total frames of a stream (known after set_pcm / set_length) */
int     lamehip_batch_frames(lamehip_batch *, int stream);
/* D2H of one stream's payload + host bit packing; returns bytes or <0 */
long    lamehip_batch_pack(lamehip_batch *, int stream, unsigned char *out, long out_size);
/* one stream as a complete file image: final Xing/Info + LAME tag frame, then the audio frames */
long    lamehip_batch_pack_tagged(lamehip_batch *, int stream, unsigned char *out, long out_size);
/* the same for all streams with `nthreads' host threads (streams are independent; the packer is
 * serial per stream): stream s at out + s * out_stride, sizes[s] = bytes or a negative code */
int     lamehip_batch_pack_all(lamehip_batch *, int nthreads, unsigned char *out, long out_stride, long *sizes);
/* Bit packing on the device: with this switched on (before lamehip_batch_encode) the kernel also
 * assembles every stream's MP3 bytes in HBM -- headers, side information, Huffman data, reservoir
 * back pointers, final padding (reference bitstream.c:format_bitstream / flush_bitstream) -- and
 * lamehip_batch_get_bytes copies them out; the host packer is not involved.  Same bytes as
 * lamehip_batch_pack. */
int     lamehip_batch_set_device_packing(lamehip_batch *, int on);
long    lamehip_batch_get_bytes(lamehip_batch *, int stream, unsigned char *out, long out_size);
int     lamehip_batch_get_bytes_all(lamehip_batch *, unsigned char *out, long out_stride, long *sizes);
/* Pipelined use (several batches in flight, each on its own HIP stream; replaces the seam of the reference's
 * frontend loop lame_encode_buffer -> fwrite, frontend/lame_main.c:449-520, for many streams at once):
 *   lamehip_batch_pcm_host_ptr   pinned mirror of the s16 pool, short[stream][2][capacity]; write the samples there
 *                                (then lamehip_batch_set_length + lamehip_batch_mark_pcm) or let lamehip_batch_set_pcm
 *                                copy them there -- NULL for a batch that converts the sample rate on the host
 *                                (lamehip_batch_set_device_resampling);
 *   lamehip_batch_upload         one asynchronous H2D copy of what changed (lamehip_batch_encode does it if pending);
 *   lamehip_batch_fetch          after lamehip_batch_encode of a device-packed batch: bytes and per-stream sizes start
 *                                their way to pinned host memory behind the kernel, asynchronously;
 *   lamehip_batch_bytes_ptr      waits for them; stream's bytes in place (valid until the next encode), returns their
 *                                number or a negative code. */
short  *lamehip_batch_pcm_host_ptr(lamehip_batch *);
int     lamehip_batch_mark_pcm(lamehip_batch *, int stream);
int     lamehip_batch_upload(lamehip_batch *);
int     lamehip_batch_fetch(lamehip_batch *);
long    lamehip_batch_bytes_ptr(lamehip_batch *, int stream, const unsigned char **bytes);
/* tag frame + audio frames, like lamehip_batch_pack_tagged, from the device-packed bytes */
long    lamehip_batch_get_bytes_tagged(lamehip_batch *, int stream, unsigned char *out, long out_size);
/* Tagging on the device, on top of device packing: with this switched on (before lamehip_batch_encode; it may be switched
 * between launches) one more kernel behind the encode kernel writes every stream's final Xing/Info + LAME tag frame into
 * HBM, directly in front of the stream's audio bytes -- the music CRC over the bytes, the seek table, the counts, the frame's
 * own CRCs (reference VbrTag.c: lame_get_lametag_frame; csrc/lh_tag.hip) --, and lamehip_batch_fetch brings complete file
 * images home, contiguous and ready to be written to disk:
 *   lamehip_batch_image_ptr      like lamehip_batch_bytes_ptr: waits for the fetch; the stream's image -- tag frame, then
 *                                audio -- in place in the pinned buffer (valid until the next encode), returns its length,
 *                                LAMEHIP_ERR_PAYLOAD when the device packer reported a status, or another negative code;
 *   lamehip_batch_get_images_all like lamehip_batch_get_bytes_all: image s at out + s * out_stride, sizes[s] = bytes or a
 *                                negative code;
 *   lamehip_batch_get_bytes_tagged  returns the same image, copied from HBM instead of made on the host.
 * The images are those of lamehip_batch_pack_tagged, byte for byte (a radio gain measured by lamehip_batch_set_replaygain is
 * put into the image when it is handed out); when the tag does not fit a frame they are the audio alone, as there.
 * lamehip_batch_get_bytes / _get_bytes_all / _bytes_ptr return the audio alone, as before.  Returns -1 unless the batch packs
 * on the device (lamehip_batch_set_device_packing first), on an incremental batch and behind
 * lamehip_batch_set_incremental_packing (whose tag frames are lamehip_batch_set_incremental_tagging's); a failed allocation returns
 * LAMEHIP_ERR_DEVICE and leaves the batch as it was.  Off (the default): launches, layouts and bytes are what they were. */
int     lamehip_batch_set_device_tagging(lamehip_batch *, int on);
long    lamehip_batch_image_ptr(lamehip_batch *, int stream, const unsigned char **image);
int     lamehip_batch_get_images_all(lamehip_batch *, unsigned char *out, long out_stride, long *sizes);
/* HIP-event time of the tag kernel of the last lamehip_batch_encode in ms (after lamehip_batch_sync; events of its own: not
 * part of lamehip_batch_last_kernel_ms or of its parts); 0 when the kernel did not run.  On a batch with
 * lamehip_batch_set_incremental_tagging: of the tag launch of the last lamehip_batch_encode_available / _finish. */
float   lamehip_batch_last_tag_ms(lamehip_batch *);
/* Tag frames for an incremental batch that packs on the device.  Accepted only with lamehip_batch_set_incremental_packing on
 * and only before any PCM, length, mirror or append has been handed over (-1 otherwise, lamehip_last_error() names the call);
 * on = 0 before the first append puts the batch back as it was; an allocation failure returns LAMEHIP_ERR_DEVICE and leaves
 * the batch as it was.  While it is on, lamehip_batch_set_incremental_packing(b, 0) is refused.
 * Every stream carries a small record in HBM (csrc/lh_tag.h: LhTagCarry): the music CRC over the bytes of its slice that
 * are final, and lh_tag_add_frame's bookkeeping -- frames, the bag of seek points, its sampling distance, the sum, the last
 * frame's mode extension.  Behind every round's drain launches ONE more launch (csrc/lh_tag.hip: lh_tag_resume_kernel, a
 * workgroup per stream) moves it on: the CRC over the round's new final bytes [crc_upto, P) -- read once, in the round they
 * become final --, joined to the carried one, and the round's LhFrameOut records into the bag.  A stream the round brought
 * nothing leaves at once; a round without a complete frame makes no launch.  Behind the flush the kernel makes every stream's
 * final Xing/Info + LAME frame from the carry, and the frames come home to pinned memory with the final round's table.
 * The drains are unchanged: they hand out the audio bytes lame_encode_buffer returns with bWriteVbrTag off, no placeholder.
 * The caller reserves lamehip_batch_tag_size bytes at the head of the file, as the reference's frontend does with its zero
 * frame, and writes the tag there at the end:
 *   lamehip_batch_tag_size       the frame's length for the batch's settings, constant from the moment the switch is on; 0
 *                                when the tag does not fit a frame (the batch then has no tags, as on the one-shot path) or
 *                                the switch is off
 *   lamehip_batch_tag_ptr        after lamehip_batch_finish, or after the round that ended the stream alone
 *                                (lamehip_batch_end_stream): stream's final tag frame in place in the pinned buffer (valid
 *                                until lamehip_batch_reset or the slot's lamehip_batch_restart_stream), returns its length;
 *                                -1 before, LAMEHIP_ERR_PAYLOAD for a stream whose packer or drain reported a status
 *   lamehip_batch_get_tags_all   frame s at out + s * out_stride, sizes[s] = bytes or a negative code (a stream that has
 *                                not ended: -1); -1 while no stream has ended
 * The frame is, byte for byte, the one lamehip_batch_pack_tagged / _get_bytes_tagged put in front of the same stream on a
 * one-shot batch fed the same samples.  With lamehip_batch_set_incremental_replaygain on, the radio gain is put into the frame
 * when it is handed out.  lamehip_batch_reset zeroes the carry.  Off (the default): launches, layouts and bytes of every path
 * are what they were. */
int     lamehip_batch_set_incremental_tagging(lamehip_batch *, int on);
int     lamehip_batch_tag_size(lamehip_batch *);
long    lamehip_batch_tag_ptr(lamehip_batch *, int stream, const unsigned char **frame);
int     lamehip_batch_get_tags_all(lamehip_batch *, unsigned char *out, long out_stride, long *sizes);
/* test accessor: the device packer's byte pool in HBM as the last lamehip_batch_reserve / lamehip_batch_encode left it (with
 * device tagging the tag frames' room is part of it) and its size in bytes; NULL when there is none */
void   *lamehip_batch_bytes_device_ptr(lamehip_batch *, long long *size);
/* raw payload access for tests: copies frames [0, n) of a stream (LhFrameOut[]) */
int     lamehip_batch_get_frames(lamehip_batch *, int stream, void *frames_out, int max_frames);
/* debug aid: raw per-stream carried state (LhStreamState, csrc/lh_device.h) */
int     lamehip_batch_get_state(lamehip_batch *, int stream, void *out, int size);
int     lamehip_get_state(const lame_t, void *out, int size);   /* same for a single-stream handle */
/* allocate what a launch of the batch's present streams needs (payload, analysis pool, byte pool) now rather than in the first
 * lamehip_batch_encode */
int     lamehip_batch_reserve(lamehip_batch *);
/* elapsed GPU time of the last lamehip_batch_encode in ms (HIP events on the batch stream) */
float   lamehip_batch_last_kernel_ms(lamehip_batch *);
/* the same launch kernel by kernel: a batch's frames go through the split pipeline -- analysis kernels over all frames at
 * once (attack detection, FHTs, spectra, masking up to the recurrences: csrc/lh_analysis.hip), the sub-band kernel
 * (polyphase + MDCT: csrc/lh_subband.hip), then the per-stream encode kernel -- parts3[0..2] = their times in ms.  Returns 1,
 * or 0 when the launch was the single fused kernel (environment LAMEHIP_FUSED=1, or no memory for the pools). */
int     lamehip_batch_last_kernel_parts_ms(lamehip_batch *, float *parts3);
/* The analysis kernels leave 34 KB per frame for the encode kernel (81 GB at 1024 streams x 60 s).  A launch whose records do not
 * fit the device's free memory is worked through in WINDOWS of as many frames per stream as do fit -- analysis kernels, then
 * the encode kernel, window after window on the batch's HIP stream, the streams' state carried between them as between two
 * launches of an incremental batch; results are the same bytes.  Returns the number of windows of the last launch (1: all at
 * once; parts3 above are sums over the windows).  Environment LAMEHIP_MID_WINDOW=n forces windows of n frames (tuning, tests);
 * under 64 frames per window the launch takes the fused kernel instead and lamehip_last_error() says so. */
int     lamehip_batch_last_windows(lamehip_batch *);
/* waves per stream of the kernel this batch encodes with: 2 (one per channel) */
int     lamehip_batch_kernel_waves(lamehip_batch *);
int     lamehip_batch_reset(lamehip_batch *);   /* re-initialise all stream states for another run (an incremental batch: every slot, ended or not) */

/* device self-test of the wave-level primitives the kernels rely on: 0 = pass */
int     lamehip_selftest(void);
const char *lamehip_last_error(void);
/* sizeof() of the POD layouts (0 LhConfig, 1 LhTables, 2 LhFrameOut, 3 LhGranule,
 * 4 LhStreamState, 5 LhStreamDesc) this library was built with */
int     lamehip_abi_sizeof(int which);
int     lamehip_device_count(void);
/* table / config access for tests (fills LhConfig / LhTables images) */
int     lamehip_get_config(const lame_t, void *cfg_out, int size);
int     lamehip_get_tables(const lame_t, void *tab_out, int size);

#ifdef __cplusplus
}
#endif
#endif
