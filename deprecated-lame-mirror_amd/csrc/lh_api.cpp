/*
 * lh_api.cpp -- C-ABI layer of liblamehip (declared in include/lamehip.h).
 *
 * Host side only: parameter collection (the lame_set_* subset of the reference,
 * set_get.c), lame_init_params -> constants + tables -> HBM, PCM staging, kernel
 * launches (lh_kernels.hip), D2H of the side-info payload and the serial bit
 * packer (lh_bitstream.c).  The per-frame arithmetic of the hot path runs only
 * in the HIP kernels; there is no CPU implementation of it in this library.
 *
 * This file holds the lame_* handle API the reference's frontend links against; the lamehip_batch_* API is in
 * lh_batch.cpp, what the two share in lh_api_int.h.
 */
#include "lh_api_int.h"

__thread char g_err[512] = "";

extern "C" const char *
lamehip_last_error(void)
{
    return g_err;
}

extern "C" int
lamehip_device_count(void)
{
    int     n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

/* the reference's default message sink (util.c:707-716) */
static void
report_to_stderr(const char *format, va_list ap)
{
    (void) vfprintf(stderr, format, ap);
    fflush(stderr);
}

static void
report_through(lame_report_function f, const char *format, ...)
{
    va_list ap;
    if (!f)
        return;
    va_start(ap, format);
    f(format, ap);
    va_end(ap);
}

/* a failed call on a handle: what lamehip_last_error() holds also goes to the handle's errorf */
static int
report_failure(lame_t g, int rc)
{
    if (rc < 0 && g && g_err[0])
        report_through(g->report_err, "lamehip: %s\n", g_err);
    return rc;
}

extern "C" int
lame_set_errorf(lame_t g, lame_report_function f)
{
    if (!valid(g))
        return -1;
    g->report_err = f;
    return 0;
}

extern "C" int
lame_set_debugf(lame_t g, lame_report_function f)
{
    if (!valid(g))
        return -1;
    g->report_dbg = f;
    return 0;
}

extern "C" int
lame_set_msgf(lame_t g, lame_report_function f)
{
    if (!valid(g))
        return -1;
    g->report_msg = f;
    return 0;
}

extern "C" lame_t
lame_init(void)
{
    lame_t  g = new(std::nothrow) lame_global_struct();
    if (!g)
        return nullptr;
    g->report_err = g->report_dbg = g->report_msg = report_to_stderr;
    lh_params_default(&g->p);
    return g;
}

#define SETTER(name, field, type) \
    extern "C" int name(lame_t g, type v) { if (!valid(g)) return -1; g->field = (int) v; return 0; }
#define GETTER(name, expr, type) \
    extern "C" type name(const lame_t g) { if (!valid(g)) return (type) 0; return (type) (expr); }

SETTER(lame_set_in_samplerate, p.samplerate, int)
GETTER(lame_get_in_samplerate, g->p.samplerate, int)
SETTER(lame_set_num_channels, p.channels, int)
GETTER(lame_get_num_channels, g->p.channels, int)
SETTER(lame_set_out_samplerate, out_samplerate, int)
GETTER(lame_get_out_samplerate, g->inited ? g->cfg.samplerate : g->out_samplerate, int)
SETTER(lame_set_brate, p.brate, int)
GETTER(lame_get_brate, g->inited ? g->cfg.avg_bitrate : g->p.brate, int)
SETTER(lame_set_quality, p.quality, int)
GETTER(lame_get_quality, g->inited ? g->cfg.quality : g->p.quality, int)
SETTER(lame_set_bWriteVbrTag, write_vbr_tag, int)
GETTER(lame_get_bWriteVbrTag, g->write_vbr_tag, int)

/* ---- the frontend's tuning switches (reference set_get.c; semantics in lh_host_init.c:config_apply_tuning) ---- */
#define FSETTER(name, field) \
    extern "C" int name(lame_t g, float v) { if (!valid(g)) return -1; g->p.field = v; return 0; }
#define FGETTER(name, field) \
    extern "C" float name(const lame_t g) { if (!valid(g)) return 0; return g->p.field; }
SETTER(lame_set_ATHtype, p.ATHtype, int)                /* lame.h:502 */
GETTER(lame_get_ATHtype, g->inited ? g->cfg.ATHtype : g->p.ATHtype, int)
FSETTER(lame_set_ATHcurve, ATHcurve)
FGETTER(lame_get_ATHcurve, ATHcurve)
FSETTER(lame_set_ATHlower, ATH_lower_db)                /* lame.h:506 */
FGETTER(lame_get_ATHlower, ATH_lower_db)
SETTER(lame_set_athaa_type, p.athaa_type, int)          /* lame.h:510 */
GETTER(lame_get_athaa_type, g->p.athaa_type, int)
FSETTER(lame_set_athaa_sensitivity, athaa_sensitivity)  /* lame.h:521 */
FGETTER(lame_get_athaa_sensitivity, athaa_sensitivity)
SETTER(lame_set_ATHonly, p.ATHonly, int)                /* lame.h:490 */
GETTER(lame_get_ATHonly, g->p.ATHonly, int)
SETTER(lame_set_ATHshort, p.ATHshort, int)              /* lame.h:494 */
GETTER(lame_get_ATHshort, g->p.ATHshort, int)
SETTER(lame_set_noATH, p.noATH, int)                    /* lame.h:498 */
GETTER(lame_get_noATH, g->p.noATH, int)
SETTER(lame_set_highpassfreq, p.highpassfreq, int)      /* lame.h:477 */
GETTER(lame_get_highpassfreq, g->p.highpassfreq, int)
SETTER(lame_set_highpasswidth, p.highpasswidth, int)    /* lame.h:480 */
GETTER(lame_get_highpasswidth, g->p.highpasswidth, int)
SETTER(lame_set_exp_nspsytune, p.exp_nspsytune, int)    /* lame.h:421 */
GETTER(lame_get_exp_nspsytune, g->p.exp_nspsytune, int)
SETTER(lame_set_experimentalY, p.experimentalY, int)    /* lame.h:413 */
GETTER(lame_get_experimentalY, g->p.experimentalY, int)
SETTER(lame_set_experimentalZ, p.experimentalZ, int)    /* lame.h:417 */
GETTER(lame_get_experimentalZ, g->p.experimentalZ, int)
FSETTER(lame_set_compression_ratio, compression_ratio)  /* lame.h:355 */
extern "C" float
lame_get_compression_ratio(const lame_t g)
{
    if (!valid(g))
        return 0;
    return g->inited ? g->cfg.compression_ratio : g->p.compression_ratio;
}

extern "C" void
lame_set_msfix(lame_t g, double msfix)                  /* lame.h:424 */
{
    if (valid(g))
        g->p.msfix = (float) msfix;
}

extern "C" float
lame_get_msfix(const lame_t g)
{
    return valid(g) ? g->p.msfix : 0;
}

extern "C" int
lame_set_interChRatio(lame_t g, float ratio)            /* lame.h:543: 0 .. 1 */
{
    if (!valid(g) || !(0 <= ratio && ratio <= 1.0))
        return -1;
    g->p.interChRatio = ratio;
    return 0;
}
FGETTER(lame_get_interChRatio, interChRatio)

extern "C" int
lame_set_useTemporal(lame_t g, int on)                  /* lame.h:539: 0 / 1 */
{
    if (!valid(g) || on < 0 || on > 1)
        return -1;
    g->p.useTemporal = on;
    return 0;
}
GETTER(lame_get_useTemporal, g->p.useTemporal, int)

extern "C" int
lame_set_free_format(lame_t g, int on)                  /* lame.h:292: accepted here, refused by lame_init_params */
{
    if (!valid(g) || on < 0 || on > 1)
        return -1;
    g->p.free_format = on;
    return 0;
}
GETTER(lame_get_free_format, g->p.free_format, int)

/* switches of the reference that have nothing to act on in this library: the decoder (decode_only,
 * decode_on_the_fly), ReplayGain analysis, assembler variants.  Their setters take the "off" value and refuse
 * the "on" value; the getters report "off" / 0 like a reference build without those parts. */
extern "C" int lame_set_decode_only(lame_t g, int v) { return (valid(g) && v == 0) ? 0 : -1; }       /* lame.h:244 */
extern "C" int lame_get_decode_only(const lame_t) { return 0; }
extern "C" int lame_set_decode_on_the_fly(lame_t, int) { return -1; }       /* (a reference without DECODE_ON_THE_FLY) */
extern "C" int lame_get_decode_on_the_fly(const lame_t) { return 0; }
/* the frontend's default (--replaygain-fast): the input's radio gain is measured on the host beside the encode
 * (lh_replaygain.c) and stored in the LAME tag */
extern "C" int
lame_set_findReplayGain(lame_t g, int on)               /* lame.h:296 */
{
    if (!valid(g) || on < 0 || on > 1)
        return -1;
    g->find_replaygain = on;
    return 0;
}
GETTER(lame_get_findReplayGain, g->find_replaygain, int)
GETTER(lame_get_RadioGain, g->tag.radio_gain, int)
extern "C" int lame_get_AudiophileGain(const lame_t) { return 0; }
extern "C" float lame_get_PeakSample(const lame_t) { return 0; }
extern "C" int lame_get_noclipGainChange(const lame_t) { return 0; }
extern "C" float lame_get_noclipScale(const lame_t) { return 0; }
extern "C" int lame_set_asm_optimizations(lame_t g, int optim, int) { return valid(g) ? optim : -1; } /* lame.h:360 */
SETTER(lame_set_nogap_total, nogap_total, int)          /* lame.h:326: bookkeeping of the frontend's --nogap */
GETTER(lame_get_nogap_total, g->nogap_total, int)
SETTER(lame_set_nogap_currentindex, nogap_current, int)
GETTER(lame_get_nogap_currentindex, g->nogap_current, int)

/* reference lame.c: bitrate_table[version][index] */
extern "C" int
lame_get_bitrate(int mpeg_version, int table_index)     /* lame.h:1290 */
{
    static const int t[3][16] = {
        {0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, -1},
        {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, -1},
        {0, 8, 16, 24, 32, 40, 48, 56, 64, -1, -1, -1, -1, -1, -1, -1}
    };
    if (0 <= mpeg_version && mpeg_version <= 2 && 0 <= table_index && table_index <= 15)
        return t[mpeg_version][table_index];
    return -1;
}

extern "C" int
lame_get_samplerate(int mpeg_version, int table_index)  /* lame.h:1291 */
{
    static const int t[3][4] = { {22050, 24000, 16000, -1}, {44100, 48000, 32000, -1}, {11025, 12000, 8000, -1} };
    if (0 <= mpeg_version && mpeg_version <= 2 && 0 <= table_index && table_index <= 3)
        return t[mpeg_version][table_index];
    return -1;
}

/* what this library answers where the reference names itself (version.c): the reference's numbers, since the
 * streams -- tag frame included -- are the reference's */
extern "C" const char *get_lame_version(void) { return "3.99.5"; }
extern "C" const char *get_lame_short_version(void) { return "3.99.5"; }
extern "C" const char *get_lame_very_short_version(void) { return "LAME3.99r"; }
extern "C" const char *get_psy_version(void) { return "1.0"; }
extern "C" const char *get_lame_url(void) { return "http://lame.sf.net"; }
extern "C" const char *get_lame_os_bitness(void) { return sizeof(void *) == 8 ? "64bits" : sizeof(void *) == 4 ? "32bits" : ""; }

/* lame_print_config / lame_print_internals (lame.h:678, 679): the settings as this library resolved them, through
 * the handle's msgf (the reference's wording is not reproduced; the frontend only passes the text on) */
extern "C" void
lame_print_config(const lame_t g)
{
    if (!valid(g) || !g->inited)
        return;
    report_through(g->report_msg, "liblamehip (MI355X): %d Hz -> %d Hz, %s, %s, quality %d, lowpass %d Hz\n", g->p.samplerate,
                   g->cfg.samplerate, g->cfg.mode == LH_MODE_MONO ? "mono" : g->cfg.mode == LH_MODE_JOINT_STEREO ? "joint stereo" :
                   g->cfg.mode == LH_MODE_DUAL ? "dual channel" : "stereo",
                   g->cfg.vbr == 0 ? "CBR" : g->cfg.vbr == 3 ? "ABR" : g->cfg.vbr == 2 ? "VBR (old)" : "VBR (new)", g->cfg.quality, g->cfg.lowpassfreq);
}

extern "C" void
lame_print_internals(const lame_t g)
{
    if (!valid(g) || !g->inited)
        return;
    report_through(g->report_msg, "liblamehip internals: bitrate %d kb/s (index %d), noise shaping %d / amp %d / stop %d, "
                   "best huffman %d, msfix %g, ATH type %d curve %g offset %g dB, temporal masking %d, short blocks %d\n",
                   g->cfg.avg_bitrate, g->cfg.bitrate_index, g->cfg.noise_shaping, g->cfg.noise_shaping_amp,
                   g->cfg.noise_shaping_stop, g->cfg.use_best_huffman, (double) g->cfg.msfix, g->cfg.ATHtype,
                   (double) g->cfg.ATHcurve, (double) g->cfg.ATH_offset_db, g->cfg.use_temporal_masking, g->cfg.short_blocks);
}

extern "C" int
lame_set_mode(lame_t g, MPEG_mode m)
{
    if (!valid(g))
        return -1;
    if ((int) m < 0 || m >= MAX_INDICATOR)
        return -1;
    g->p.mode = (m == NOT_SET) ? -1 : (int) m;
    return 0;
}

extern "C" MPEG_mode
lame_get_mode(const lame_t g)
{
    if (!valid(g))
        return NOT_SET;
    if (g->inited)
        return (MPEG_mode) g->cfg.mode;
    return g->p.mode < 0 ? NOT_SET : (MPEG_mode) g->p.mode;
}

extern "C" int
lame_set_VBR(lame_t g, vbr_mode v)
{
    if (!valid(g))
        return -1;
    g->p.vbr = (int) v;
    return 0;
}

extern "C" vbr_mode
lame_get_VBR(const lame_t g)
{
    return valid(g) ? (vbr_mode) g->p.vbr : vbr_off;
}

extern "C" int
lame_set_VBR_q(lame_t g, int q)
{
    int     ret = 0;
    if (!valid(g))
        return -1;
    if (q < 0) {                /* reference set_get.c:1127-1141: clamps and reports -1 */
        ret = -1;
        q = 0;
    }
    if (q > 9) {
        ret = -1;
        q = 9;
    }
    g->p.vbr_q = q;
    g->p.vbr_q_frac = 0;
    return ret;
}

/* --preset / lame_set_preset (reference set_get.c:2158-2166, presets.c:319-420): the named presets
 * and V0..V9 select the new VBR loop's quality, 8..320 an ABR mean, INSANE is CBR 320.  Applied at
 * call time like the reference, so later lame_set_* calls still override. */
extern "C" int
lame_set_preset(lame_t g, int preset)
{
    if (!valid(g))
        return -1;
    switch (preset) {
    case 1000:                 /* R3MIX */
        preset = 470;
        g->p.vbr = 4;
        break;
    case 1006:                 /* MEDIUM, MEDIUM_FAST */
    case 1007:
        preset = 460;
        g->p.vbr = 4;
        break;
    case 1001:                 /* STANDARD, STANDARD_FAST */
    case 1004:
        preset = 480;
        g->p.vbr = 4;
        break;
    case 1002:                 /* EXTREME, EXTREME_FAST */
    case 1005:
        preset = 500;
        g->p.vbr = 4;
        break;
    case 1003:                 /* INSANE */
        g->p.vbr = 0;
        g->p.brate = g->p.abr_kbps = 320;
        g->p.preset_kbps = (!g->p.preset_kbps || g->p.preset_kbps == 320) ? 320 : -1;   /* -1: two different ones */
        g->p.scale *= lh_abr_preset_scale(320);
        g->preset_vbr = 0;
        return 320;
    }
    if (preset >= 410 && preset <= 500 && preset % 10 == 0) {   /* V9 .. V0 */
        g->p.vbr_q = (500 - preset) / 10;
        g->p.vbr_q_frac = 0;
        g->preset_vbr = 1;      /* its tunings are the VBR loop's: not combined with CBR / ABR here */
        return preset;
    }
    if (8 <= preset && preset <= 320) {
        g->p.vbr = 3;
        g->p.abr_kbps = g->p.brate = preset;
        /* (its row's tuning values stay when the bitrate changes afterwards: lh_host_init.c) */
        g->p.preset_kbps = (!g->p.preset_kbps || g->p.preset_kbps == preset) ? preset : -1;
        g->p.scale *= lh_abr_preset_scale(preset);      /* and once more in lame_init_params, like the reference */
        g->preset_vbr = 0;
    }
    return preset;
}

/* -V n.f (reference set_get.c:1155-1175) */
extern "C" int
lame_set_VBR_quality(lame_t g, float q)
{
    int     ret = 0;
    if (!valid(g))
        return -1;
    if (0 > q) {
        ret = -1;
        q = 0;
    }
    if (9.999 < q) {
        ret = -1;
        q = 9.999;
    }
    g->p.vbr_q = (int) q;
    g->p.vbr_q_frac = q - g->p.vbr_q;
    return ret;
}

extern "C" float
lame_get_VBR_quality(const lame_t g)
{
    return valid(g) ? g->p.vbr_q + g->p.vbr_q_frac : 0;
}

SETTER(lame_set_VBR_min_bitrate_kbps, p.vbr_min_kbps, int)
GETTER(lame_get_VBR_min_bitrate_kbps, g->inited && g->cfg.vbr ? lh_tag_kbps(g->cfg.version, g->cfg.vbr_min_bitrate_index) : g->p.vbr_min_kbps, int)
SETTER(lame_set_VBR_max_bitrate_kbps, p.vbr_max_kbps, int)
GETTER(lame_get_VBR_max_bitrate_kbps, g->inited && g->cfg.vbr ? lh_tag_kbps(g->cfg.version, g->cfg.vbr_max_bitrate_index) : g->p.vbr_max_kbps, int)
SETTER(lame_set_VBR_hard_min, p.vbr_hard_min, int)
GETTER(lame_get_VBR_hard_min, g->p.vbr_hard_min, int)

GETTER(lame_get_VBR_q, g->inited ? g->cfg.vbr_q : g->p.vbr_q, int)
SETTER(lame_set_force_ms, p.force_ms, int)
GETTER(lame_get_force_ms, g->p.force_ms, int)
SETTER(lame_set_disable_reservoir, p.disable_reservoir, int)
GETTER(lame_get_disable_reservoir, g->p.disable_reservoir, int)
SETTER(lame_set_error_protection, p.error_protection, int)
GETTER(lame_get_error_protection, g->p.error_protection, int)
SETTER(lame_set_copyright, p.copyright, int)
GETTER(lame_get_copyright, g->p.copyright, int)
SETTER(lame_set_original, p.original, int)
GETTER(lame_get_original, g->p.original, int)
SETTER(lame_set_emphasis, p.emphasis, int)
GETTER(lame_get_emphasis, g->p.emphasis, int)
SETTER(lame_set_extension, p.extension, int)
GETTER(lame_get_extension, g->p.extension, int)
SETTER(lame_set_strict_ISO, p.strict_ISO, int)
GETTER(lame_get_strict_ISO, g->p.strict_ISO, int)
SETTER(lame_set_lowpassfreq, p.lowpassfreq, int)
GETTER(lame_get_lowpassfreq, g->inited ? g->cfg.lowpassfreq : g->p.lowpassfreq, int)
SETTER(lame_set_lowpasswidth, p.lowpasswidth, int)
GETTER(lame_get_lowpasswidth, g->p.lowpasswidth, int)

extern "C" int
lame_set_scale(lame_t g, float v)
{
    if (!valid(g))
        return -1;
    g->p.scale = v;
    return 0;
}

extern "C" int
lame_set_scale_left(lame_t g, float v)
{
    if (!valid(g))
        return -1;
    g->p.scale_left = v;
    return 0;
}

extern "C" int
lame_set_scale_right(lame_t g, float v)
{
    if (!valid(g))
        return -1;
    g->p.scale_right = v;
    return 0;
}

/* short block switches (reference set_get.c:1650-1846) */
extern "C" int
lame_set_allow_diff_short(lame_t g, int v)
{
    if (!valid(g))
        return -1;
    g->p.short_blocks = v ? 0 : 1;
    return 0;
}

extern "C" int
lame_set_no_short_blocks(lame_t g, int v)
{
    if (!valid(g) || v < 0 || v > 1)
        return -1;
    g->p.short_blocks = v ? 2 : 0;
    return 0;
}

extern "C" int
lame_set_force_short_blocks(lame_t g, int v)
{
    if (!valid(g) || v < 0 || v > 1)
        return -1;
    if (v == 1)
        g->p.short_blocks = 3;
    else if (g->p.short_blocks == 3)
        g->p.short_blocks = 0;
    return 0;
}

SETTER(lame_set_VBR_mean_bitrate_kbps, p.abr_kbps, int)
GETTER(lame_get_VBR_mean_bitrate_kbps, g->inited ? g->cfg.vbr_avg_bitrate_kbps : g->p.abr_kbps, int)

GETTER(lame_get_framesize, g->inited ? fs_of(g->cfg) : 576 * 2, int)
GETTER(lame_get_frameNum, g->frames_done - g->frame_num_base, int)
GETTER(lame_get_encoder_delay, LH_ENCDELAY, int)
GETTER(lame_get_encoder_padding, g->enc_padding, int)
/* ENCDELAY + POSTDELAY + samples taken in - samples encoded; 0 after the flush (reference lame.c:1737-1766, 2117) */
GETTER(lame_get_mf_samples_to_encode, (!g->inited || g->flushed) ? 0 : (int) (LH_ENCDELAY + LH_POSTDELAY + g->fed - (long long) fs_of(g->cfg) * g->frames_done), int)

extern "C" int
lame_set_num_samples(lame_t g, unsigned long n)
{
    if (!valid(g))
        return -1;
    g->num_samples = n;
    return 0;
}

extern "C" unsigned long
lame_get_num_samples(const lame_t g)
{
    return valid(g) ? g->num_samples : 0;
}

/* frames the stream will have, from the announced sample count (reference set_get.c:2120-2152) */
extern "C" int
lame_get_totalframes(const lame_t g)
{
    unsigned long n, padding;
    if (!valid(g) || !g->inited)
        return 0;
    n = g->num_samples;
    if (n == (0ul - 1ul))
        return 0;
    if (g->p.samplerate != g->cfg.samplerate && g->p.samplerate > 0) {
        double const q = (double) g->cfg.samplerate / g->p.samplerate;
        n *= q;
    }
    n += 576;
    padding = (unsigned long) fs_of(g->cfg) - (n % (unsigned long) fs_of(g->cfg));
    if (padding < 576)
        padding += (unsigned long) fs_of(g->cfg);
    n += padding;
    return (int) (n / (unsigned long) fs_of(g->cfg));
}

/* histograms over the frames encoded so far (reference lame.c:2461-2610) */
extern "C" void
lame_bitrate_kbps(const lame_t g, int bitrate_kbps[14])
{
    if (valid(g) && g->inited)
        for (int i = 0; i < 14; i++)
            bitrate_kbps[i] = lh_tag_kbps(g->inited ? g->cfg.version : 1, i + 1);
}

extern "C" void
lame_bitrate_hist(const lame_t g, int bitrate_count[14])
{
    if (valid(g) && g->inited)
        for (int i = 0; i < 14; i++)
            bitrate_count[i] = g->hist.mode[i + 1][4];
}

extern "C" void
lame_stereo_mode_hist(const lame_t g, int stmode_count[4])
{
    if (valid(g) && g->inited)
        for (int i = 0; i < 4; i++)
            stmode_count[i] = g->hist.mode[15][i];
}

extern "C" void
lame_bitrate_stereo_mode_hist(const lame_t g, int bitrate_stmode_count[14][4])
{
    if (valid(g) && g->inited)
        for (int j = 0; j < 14; j++)
            for (int i = 0; i < 4; i++)
                bitrate_stmode_count[j][i] = g->hist.mode[j + 1][i];
}

extern "C" void
lame_block_type_hist(const lame_t g, int btype_count[6])
{
    if (valid(g) && g->inited)
        for (int i = 0; i < 6; i++)
            btype_count[i] = g->hist.block[15][i];
}

extern "C" void
lame_bitrate_block_type_hist(const lame_t g, int bitrate_btype_count[14][6])
{
    if (valid(g) && g->inited)
        for (int j = 0; j < 14; j++)
            for (int i = 0; i < 6; i++)
                bitrate_btype_count[j][i] = g->hist.block[j + 1][i];
}
GETTER(lame_get_version, g->inited ? g->cfg.version : 1, int)

static int init_params_once(lame_t g);

extern "C" int
lame_init_params(lame_t g)
{
    int     rc;
    if (!valid(g))
        return -1;
    if (g->inited)
        return g->init_rc;      /* a second call reports what the first one found (also its failure) */
    g_err[0] = 0;               /* what the report callback prints is this call's, never an earlier call's */
    rc = init_params_once(g);
    if (g->inited)
        g->init_rc = rc;
    return report_failure(g, rc);
}

static int
init_params_once(lame_t g)
{
    LhInitAux aux;
    g->p.samplerate_out = g->out_samplerate;
    if (g->preset_vbr && g->p.vbr != 1 && g->p.vbr != 2 && g->p.vbr != 4) {
        snprintf(g_err, sizeof(g_err), "a V0..V9 preset without lame_set_VBR(vbr_mtrh / vbr_mt / vbr_rh) is outside the accelerated path");
        return -1;
    }
    if (g->p.preset_kbps < 0) {
        snprintf(g_err, sizeof(g_err), "two different bitrate presets (lame_set_preset 8..320 / INSANE) on one handle are outside the accelerated path");
        return -1;
    }
    if (g->p.preset_kbps && (g->preset_vbr || g->p.vbr == 1 || g->p.vbr == 2 || g->p.vbr == 4)) {
        /* e.g. --preset insane --vbr-old, --preset 192 --preset extreme: the reference then runs a VBR loop with what the
         * bitrate preset's row left in its tuning options -- a combination nobody asks for, not rebuilt here */
        snprintf(g_err, sizeof(g_err), "a bitrate preset (lame_set_preset 8..320 / INSANE) followed by a VBR mode is outside the accelerated path");
        return -1;
    }
    if (lh_config_resolve(&g->p, &g->cfg, &aux) != 0) {
        snprintf(g_err, sizeof(g_err),
                 "unsupported settings for the MI355X path (need an MPEG output rate, 1 or 2 input channels)");
        return -1;
    }
    /* (a call that failed before g->inited may be repeated: what it had allocated is reused) */
    if (!g->tab)
        g->tab = (LhTables *) malloc(sizeof(LhTables));
    if (!g->tab) {
        snprintf(g_err, sizeof(g_err), "out of memory (tables)");
        return -2;
    }
    if (lh_tables_build(&g->cfg, &aux, g->tab) != 0) {
        snprintf(g_err, sizeof(g_err), "table generation failed");
        return -1;
    }
    if (!g->bs.buf && lh_bs_init(&g->bs) != 0) {
        snprintf(g_err, sizeof(g_err), "out of memory (bit stream buffer)");
        return -2;
    }
    if (lh_rs_needed(g->p.samplerate, g->cfg.samplerate)) {
        if (!g->rs)
            g->rs = (LhResampler *) malloc(sizeof(LhResampler));
        if (!g->rs) {
            snprintf(g_err, sizeof(g_err), "out of memory (sample rate converter)");
            return -2;
        }
        lh_rs_init(g->rs, g->p.samplerate, g->cfg.samplerate);
    }
    if (g->find_replaygain) {
        if (!g->rg)
            g->rg = (LhReplayGain *) malloc(sizeof(LhReplayGain));
        if (!g->rg || lh_rg_start(g->rg, g->cfg.samplerate) != 0) {
            snprintf(g_err, sizeof(g_err), "ReplayGain analysis could not be set up");
            return -6;          /* the reference's code for it (lame.c:1264-1268) */
        }
    }
    g->inited = 1;              /* host constants are valid from here on (lamehip_get_*) */
    /* the tag frame is reserved at the head of the stream (reference InitVbrTag); when it does
     * not fit the reference silently switches it off */
    if (g->write_vbr_tag && lh_tag_init(&g->tag, &g->cfg) > 0)
        g->tag_placeholder_pending = 1;
    else
        g->write_vbr_tag = 0;
    g->tag.samplerate_in = g->p.samplerate;
    g->tag.radio_gain_on = g->find_replaygain;
    g->tag.radio_gain = 0;
    g->tag.nogap_total = g->nogap_total;
    g->tag.nogap_current = g->nogap_current;
    if (lamehip_device_count() <= 0) {
        snprintf(g_err, sizeof(g_err), "no HIP device: liblamehip has no CPU encode path");
        g->have_device = 0;
        return LAMEHIP_ERR_NODEVICE;
    }
    if (g->device < 0 && hipGetDevice(&g->device) != hipSuccess)
        g->device = 0;
    if (g->device >= lamehip_device_count()) {
        snprintf(g_err, sizeof(g_err), "lamehip_set_device: no HIP device %d", g->device);
        return LAMEHIP_ERR_NODEVICE;
    }
    {
        LhDeviceScope const on_device(g->device);
        int     rc = g->dc.upload(g->cfg, *g->tab);
        LhStreamState s0;
        if (rc)
            return rc;
        HIPCHK(g->stream.create());
        HIPCHK(g->d_state.alloc(1));
        HIPCHK(g->d_desc.alloc(1));
        lh_state_init(&s0, &g->cfg);
        HIPCHK(hipMemcpy(g->d_state.get(), &s0, sizeof(s0), hipMemcpyHostToDevice));
    }
    g->have_device = 1;
    return 0;
}

/* the reserved tag frame leaves with the first bytes the caller gets (reference lame.c:1744-1748:
 * copy_buffer(.., 0) at the start of every lame_encode_buffer call) */
static int
emit_tag_placeholder(lame_t g, unsigned char *mp3buf, int mp3buf_size, int *written)
{
    if (!g->tag_placeholder_pending)
        return 0;
    if (mp3buf_size != 0 && mp3buf_size - *written < g->tag.total_frame_size)
        return -1;
    {
        unsigned char *h = mp3buf + *written;
        *written += lh_tag_placeholder(&g->tag, &g->cfg, h);
        if (g->have_last)       /* a later file of a --nogap run: the header carries the last frame's mode extension */
            h[3] = (unsigned char) ((h[3] & 0xcf) | ((g->last_frame.mode_ext & 3) << 4));
    }
    g->tag_placeholder_pending = 0;
    return 0;
}

/* encode frames [frames_done, upto) of the single-handle stream and append the packed bytes */
static int
handle_encode_frames(lame_t g, int upto, unsigned char *mp3buf, int mp3buf_size, int *written)
{
    int const f0 = g->frames_done, nf = upto - f0;
    long long p0, p1, n;
    LhStreamDesc d;
    if (nf <= 0)
        return 0;
    /* samples touched: priming of frame 0 reaches 1152 further back (all zero there) */
    p0 = (long long) fs_of(g->cfg) * f0 - LH_MF_START - fs_of(g->cfg);
    if (p0 < g->hist_base)
        p0 = g->hist_base;
    p1 = (long long) fs_of(g->cfg) * (upto - 1) - LH_MF_START + LH_MF_NEEDED;
    if (p1 > g->fed)
        p1 = g->fed;
    n = p1 > p0 ? p1 - p0 : 0;
    /* (two planes in one buffer, each as long as half of it) */
    HIPCHK(g->d_pcm.reserve(2 * (size_t) n, 2 * 4096));
    size_t const plane = g->d_pcm.cap() / 2;
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(g->d_pcm.get(), &g->hl[(size_t) (p0 - g->hist_base)], (size_t) n * sizeof(float),
                              hipMemcpyHostToDevice, g->stream));
        HIPCHK(hipMemcpyAsync(g->d_pcm.get() + plane, &g->hr[(size_t) (p0 - g->hist_base)],
                              (size_t) n * sizeof(float), hipMemcpyHostToDevice, g->stream));
    }
    HIPCHK(g->d_out.reserve((size_t) nf, 8));
    d.pcm_l = 0;
    d.pcm_r = (long long) plane;
    d.pcm_base = p0;
    d.nsamples = g->fed;
    d.out_index = 0;
    d.frame_begin = f0;
    d.frame_end = upto;
    d.bytes_base = d.bytes_cap = 0;
    d.flush = d.mid_rel = 0;
    HIPCHK(hipMemcpyAsync(g->d_desc.get(), &d, sizeof(d), hipMemcpyHostToDevice, g->stream));
    {
        int     rc = g->dc.launch((const int16_t *) 0, g->d_pcm.get(), g->d_desc.get(), g->d_state.get(), g->d_out.get(), (uint8_t *) 0, 1,
                                  (void *) (hipStream_t) g->stream);
        if (rc)
            return set_err("kernel launch", (hipError_t) rc);
    }
    g->h_out.resize((size_t) nf);
    HIPCHK(hipMemcpyAsync(g->h_out.data(), g->d_out.get(), (size_t) nf * sizeof(LhFrameOut),
                          hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    for (int i = 0; i < nf; i++) {
        int     k;
        if (lh_bs_format_frame(&g->bs, &g->cfg, g->tab, &g->h_out[(size_t) i]) != 0) {
            int     n = snprintf(g_err, sizeof(g_err), "inconsistent device payload (packer check %d) at frame %d",
                                 g->bs.error, f0 + i);
            for (int q = 0; q < 4 && n > 0 && n < (int) sizeof(g_err); q++) {
                const LhGranule *gi = &g->h_out[(size_t) i].gr[q >> 1][q & 1];
                n += snprintf(g_err + n, sizeof(g_err) - (size_t) n, " [bv %d c1 %d gg %d bt %d ts %d/%d/%d r %d/%d]",
                              gi->big_values, gi->count1, gi->global_gain, gi->block_type, gi->table_select[0],
                              gi->table_select[1], gi->table_select[2], gi->region0_count, gi->region1_count);
            }
            return LAMEHIP_ERR_PAYLOAD;
        }
        k = lh_bs_copy(&g->bs, mp3buf + *written, mp3buf_size ? mp3buf_size - *written : 0);
        if (k < 0)
            return -1;
        /* (updateStats, reference encoder.c:156-184: the granules and channels the stream has, lh_stats.h) */
        lh_stats_count_frame(&g->hist, &g->h_out[(size_t) i], g->cfg.channels, g->cfg.mode_gr);
        if (g->write_vbr_tag) {
            lh_tag_add_frame(&g->tag, lh_tag_kbps(g->cfg.version, g->h_out[(size_t) i].bitrate_index));  /* reference encoder.c:550-551 */
            lh_tag_crc(&g->tag, mp3buf + *written, k);          /* reference bitstream.c:1082-1088 */
        }
        *written += k;
    }
    g->last_frame = g->h_out[(size_t) nf - 1];
    g->have_last = 1;
    g->frames_done = upto;
    /* drop history that no later frame (nor its priming) can touch */
    {
        long long keep = (long long) fs_of(g->cfg) * g->frames_done - LH_MF_START - 64;
        if (keep > g->hist_base) {
            size_t  drop = (size_t) (keep - g->hist_base);
            if (drop > g->hl.size())
                drop = g->hl.size();
            g->hl.erase(g->hl.begin(), g->hl.begin() + (long) drop);
            g->hr.erase(g->hr.begin(), g->hr.begin() + (long) drop);
            g->hist_base += (long long) drop;
        }
    }
    return 0;
}

/* lame_encode_buffer_template + lame_copy_inbuffer (reference lame.c:1786-1872): samples of any
 * type become sample_t through the transform matrix scaled by the type's norm; the frames that
 * became complete are encoded */
template < typename T > static int encode_buffer_impl(lame_t g, const T * l, const T * r, int nsamples, int jump,
                                                      float norm, unsigned char *mp3buf, int mp3buf_size);

template < typename T > static int
encode_buffer_any(lame_t g, const T * l, const T * r, int nsamples, int jump, float norm, unsigned char *mp3buf,
                  int mp3buf_size)
{
    g_err[0] = 0;
    return report_failure(g, encode_buffer_impl(g, l, r, nsamples, jump, norm, mp3buf, mp3buf_size));
}

template < typename T > static int
encode_buffer_impl(lame_t g, const T * l, const T * r, int nsamples, int jump, float norm, unsigned char *mp3buf,
                   int mp3buf_size)
{
    LhDeviceScope const on_device(valid(g) ? g->device : -1);
    int     written = 0, rc, avail;
    if (!valid(g) || !g->inited)
        return -3;
    if (!g->have_device)
        return LAMEHIP_ERR_NODEVICE;
    if (nsamples == 0)
        return 0;
    if (nsamples < 0)
        return -1;
    if (g->p.channels == 1)
        r = l;                  /* one input channel: buffer_r is not read (reference lame.c:1855-1866) */
    if (!l || !r)
        return 0;
    {
        /* pcm_transform: [0] = { pcm_scale, pcm_mix }, [1] = { 0, pcm_scale_r } */
        float const m00 = norm * g->cfg.pcm_scale, m01 = norm * g->cfg.pcm_mix;
        float const m10 = norm * (0.0f * g->cfg.pcm_scale), m11 = norm * g->cfg.pcm_scale_r;
        std::vector < float >&dl = g->rs ? g->tl : g->hl;
        std::vector < float >&dr = g->rs ? g->tr : g->hr;
        size_t const at = g->rs ? 0 : g->hl.size();
        dl.resize(at + (size_t) nsamples);
        dr.resize(at + (size_t) nsamples);
        for (int i = 0; i < nsamples; i++) {
            float const xl = (float) l[(size_t) i * (size_t) jump];
            float const xr = (float) r[(size_t) i * (size_t) jump];
            dl[at + (size_t) i] = xl * m00 + xr * m01;
            dr[at + (size_t) i] = xl * m10 + xr * m11;
        }
    }
    if (g->rs) {
        /* the reference's loop (lame.c:1708-1772, fill_buffer util.c:665-697): blocks of at most one
         * frame of output until the call's input is used up; every output channel sees the same
         * block boundaries */
        int     pos = 0, left = nsamples;
        while (left > 0) {
            float   blk[2][1152];
            int     used = 0, made = 0;
            for (int ch = 0; ch < g->cfg.channels; ch++)
                made = lh_rs_block(g->rs, ch, blk[ch], fs_of(g->cfg), (ch ? g->tr.data() : g->tl.data()) + pos, left, &used);
            if (g->cfg.channels == 1)
                memset(blk[1], 0, sizeof(blk[1]));
            g->hl.insert(g->hl.end(), blk[0], blk[0] + made);
            g->hr.insert(g->hr.end(), blk[1], blk[1] + made);
            if (g->rg)
                (void) lh_rg_block(g->rg, blk[0], blk[1], made, g->cfg.channels);       /* reference lame.c:1715-1720 */
            g->fed += made;
            pos += used;
            left -= used;
        }
    }
    else {
        /* (the reference's loop hands the analysis what one fill_buffer call took in: at most a frame's samples) */
        if (g->rg) {
            size_t const at = g->hl.size() - (size_t) nsamples;
            for (int pos = 0; pos < nsamples; pos += fs_of(g->cfg)) {
                int const m = nsamples - pos > fs_of(g->cfg) ? fs_of(g->cfg) : nsamples - pos;
                (void) lh_rg_block(g->rg, g->hl.data() + at + (size_t) pos, g->hr.data() + at + (size_t) pos, m, g->cfg.channels);
            }
        }
        g->fed += nsamples;
    }
    g->flushed = 0;
    /* a frame is encoded whenever 1904 samples are buffered behind the 528-sample
     * lead-in (reference lame.c:1737-1769) */
    avail = (LH_MF_START + g->fed >= mfn_of(g->cfg))
        ? (int) ((LH_MF_START + g->fed - mfn_of(g->cfg)) / fs_of(g->cfg) + 1) : 0;
    if (emit_tag_placeholder(g, mp3buf, mp3buf_size, &written))
        return -1;
    rc = handle_encode_frames(g, avail, mp3buf, mp3buf_size, &written);
    if (rc)
        return rc;
    return written;
}

extern "C" int
lame_encode_buffer(lame_t g, const short int l[], const short int r[], const int nsamples,
                   unsigned char *mp3buf, const int mp3buf_size)
{
    return encode_buffer_any(g, l, r, nsamples, 1, 1.0f, mp3buf, mp3buf_size);
}

extern "C" int
lame_encode_buffer_interleaved(lame_t g, short int pcm[], int num_samples, unsigned char *mp3buf,
                               int mp3buf_size)
{
    return encode_buffer_any(g, pcm, pcm + 1, num_samples, 2, 1.0f, mp3buf, mp3buf_size);
}

/* +/- 32768 full scale (reference lame.c:1884-1890) */
extern "C" int
lame_encode_buffer_float(lame_t g, const float l[], const float r[], const int nsamples, unsigned char *mp3buf,
                         const int mp3buf_size)
{
    return encode_buffer_any(g, l, r, nsamples, 1, 1.0f, mp3buf, mp3buf_size);
}

/* +/- 1.0 full scale (reference lame.c:1894-1930) */
extern "C" int
lame_encode_buffer_ieee_float(lame_t g, const float l[], const float r[], const int nsamples, unsigned char *mp3buf,
                              const int mp3buf_size)
{
    return encode_buffer_any(g, l, r, nsamples, 1, 32767.0f, mp3buf, mp3buf_size);
}

extern "C" int
lame_encode_buffer_interleaved_ieee_float(lame_t g, const float pcm[], const int nsamples, unsigned char *mp3buf,
                                          const int mp3buf_size)
{
    return encode_buffer_any(g, pcm, pcm + 1, nsamples, 2, 32767.0f, mp3buf, mp3buf_size);
}

extern "C" int
lame_encode_buffer_ieee_double(lame_t g, const double l[], const double r[], const int nsamples,
                               unsigned char *mp3buf, const int mp3buf_size)
{
    return encode_buffer_any(g, l, r, nsamples, 1, 32767.0f, mp3buf, mp3buf_size);
}

extern "C" int
lame_encode_buffer_interleaved_ieee_double(lame_t g, const double pcm[], const int nsamples, unsigned char *mp3buf,
                                           const int mp3buf_size)
{
    return encode_buffer_any(g, pcm, pcm + 1, nsamples, 2, 32767.0f, mp3buf, mp3buf_size);
}

/* +/- MAX_INT full scale (reference lame.c:1934-1942) */
extern "C" int
lame_encode_buffer_int(lame_t g, const int l[], const int r[], const int nsamples, unsigned char *mp3buf,
                       const int mp3buf_size)
{
    float const norm = (float) (1.0 / (1L << (8 * sizeof(int) - 16)));
    return encode_buffer_any(g, l, r, nsamples, 1, norm, mp3buf, mp3buf_size);
}

/* +/- MAX_LONG full scale (reference lame.c:1945-1953) */
extern "C" int
lame_encode_buffer_long2(lame_t g, const long l[], const long r[], const int nsamples, unsigned char *mp3buf,
                         const int mp3buf_size)
{
    float const norm = (float) (1.0 / (1L << (8 * sizeof(long) - 16)));
    return encode_buffer_any(g, l, r, nsamples, 1, norm, mp3buf, mp3buf_size);
}

/* +/- 32768 full scale in a long (reference lame.c:1956-1962) */
extern "C" int
lame_encode_buffer_long(lame_t g, const long l[], const long r[], const int nsamples, unsigned char *mp3buf,
                        const int mp3buf_size)
{
    return encode_buffer_any(g, l, r, nsamples, 1, 1.0f, mp3buf, mp3buf_size);
}

static int finish_stream(lame_t g, unsigned char *mp3buf, int size, int written);

/* lame_encode_flush with the resampler in the way (reference lame.c:2075-2120): the number of
 * frames still owed follows from the samples buffered plus the resampler's delay, and zeros are fed
 * through lame_encode_buffer -- resampler included -- in bunches sized to complete one frame at a
 * time until those frames have come out */
static int
flush_resampled(lame_t g, unsigned char *mp3buf, int size)
{
    static const short zeros[1152] = { 0 };
    double const ratio = g->rs->ratio;
    /* mf_samples_to_encode - POSTDELAY, with mf_samples_to_encode = ENCDELAY + POSTDELAY + fed - 1152 frames */
    int     owed = (int) (576 + g->fed - (long long) fs_of(g->cfg) * g->frames_done);
    int     padding, frames_left, written = 0;
    owed += 16. / ratio;
    padding = fs_of(g->cfg) - (owed % fs_of(g->cfg));
    if (padding < 576)
        padding += fs_of(g->cfg);
    g->enc_padding = padding;
    frames_left = (owed + padding) / fs_of(g->cfg);
    while (frames_left > 0) {
        int const before = g->frames_done;
        int     bunch = mfn_of(g->cfg) - (int) (LH_MF_START + g->fed - (long long) fs_of(g->cfg) * g->frames_done);
        int     k;
        bunch *= ratio;
        if (bunch > 1152)
            bunch = 1152;
        if (bunch < 1)
            bunch = 1;
        k = encode_buffer_any(g, zeros, zeros, bunch, 1, 1.0f, mp3buf + written, size ? size - written : 0);
        if (k < 0)
            return k;
        written += k;
        frames_left -= (g->frames_done != before) ? 1 : 0;
    }
    return finish_stream(g, mp3buf, size, written);
}

extern "C" int
lame_encode_flush(lame_t g, unsigned char *mp3buf, int size)
{
    LhDeviceScope const on_device(valid(g) ? g->device : -1);
    int     written = 0, rc, total;
    if (!valid(g) || !g->inited)
        return -3;
    if (!g->have_device)
        return LAMEHIP_ERR_NODEVICE;
    if (g->flushed)
        return 0;               /* reference lame.c:2076-2079 */
    if (g->rs)
        return flush_resampled(g, mp3buf, size);
    if (g->rg) {
        /* the reference flushes by feeding zeros through lame_encode_buffer, (mf_needed - mf_size) <= 1152 at a time,
         * until the frames it owes are out (lame.c:2093-2117); the analysis hears those zeros */
        static const float zeros[1152] = { 0 };
        long long fed = g->fed;
        int     frames = g->frames_done;
        int const owed = (int) (576 + fed - (long long) fs_of(g->cfg) * frames);
        int     padding = fs_of(g->cfg) - (owed % fs_of(g->cfg)), frames_left;
        if (padding < 576)
            padding += fs_of(g->cfg);
        frames_left = (owed + padding) / fs_of(g->cfg);
        while (frames_left > 0) {
            int     bunch = mfn_of(g->cfg) - (int) (LH_MF_START + fed - (long long) fs_of(g->cfg) * frames);
            bunch = bunch > 1152 ? 1152 : (bunch < 1 ? 1 : bunch);
            (void) lh_rg_block(g->rg, zeros, zeros, bunch, g->cfg.channels);
            fed += bunch;
            if (LH_MF_START + fed - (long long) fs_of(g->cfg) * frames >= mfn_of(g->cfg)) {
                frames++;
                frames_left--;
            }
        }
    }
    total = lh_total_frames_fs((long) g->fed, fs_of(g->cfg));
    g->enc_padding = lh_end_padding_fs((long) g->fed, fs_of(g->cfg));     /* reference lame.c:2088-2091 */
    if (emit_tag_placeholder(g, mp3buf, size, &written))
        return -1;
    rc = handle_encode_frames(g, total, mp3buf, size, &written);
    if (rc)
        return rc;
    return finish_stream(g, mp3buf, size, written);
}

/* pad the last frame out and hand over the rest of the bytes (reference lame.c:2122-2160) */
static int
finish_stream(lame_t g, unsigned char *mp3buf, int size, int written)
{
    int     k;
    lh_bs_flush(&g->bs, &g->cfg, g->have_last ? &g->last_frame : nullptr);
    k = lh_bs_copy(&g->bs, mp3buf + written, size ? size - written : 0);
    if (k < 0)
        return -1;
    if (g->rg)
        g->tag.radio_gain = lh_rg_finish(g->rg);        /* save_gain_values, reference lame.c:1565-1580 */
    if (g->write_vbr_tag)
        lh_tag_crc(&g->tag, mp3buf + written, k);
    written += k;
    g->flushed = 1;
    /* the reference zeroes the reservoir after padding out the last frame (bitstream.c:886-888) */
    {
        LhStreamState s;
        if (hipMemcpy(&s, g->d_state.get(), sizeof(s), hipMemcpyDeviceToHost) == hipSuccess) {
            s.ResvSize = 0;
            s.main_data_begin = 0;
            (void) hipMemcpy(g->d_state.get(), &s, sizeof(s), hipMemcpyHostToDevice);
        }
    }
    return written;
}

/* --nogap: close the bitstream at a file boundary without draining the sample buffers (reference
 * lame.c:1988-2001): the pending frames are padded out and the reservoir starts from zero, so the
 * pieces decode on their own and, concatenated, without a gap. */
extern "C" int
lame_encode_flush_nogap(lame_t g, unsigned char *mp3buf, int size)
{
    LhDeviceScope const on_device(valid(g) ? g->device : -1);
    int     was, k;
    if (!valid(g) || !g->inited)
        return -3;
    if (!g->have_device)
        return LAMEHIP_ERR_NODEVICE;
    was = g->flushed;
    k = finish_stream(g, mp3buf, size, 0);
    g->flushed = was;
    return k;
}

/* start the next file of a --nogap run: frame counter, histograms and a fresh tag frame
 * (reference lame.c:2006-2035) */
extern "C" int
lame_init_bitstream(lame_t g)
{
    if (!valid(g) || !g->inited)
        return -3;
    g->frame_num_base = g->frames_done;
    memset(&g->hist, 0, sizeof(g->hist));
    {
        uint16_t const crc = g->tag.music_crc;  /* the reference's music CRC runs on across the files */
        if (g->write_vbr_tag && lh_tag_init(&g->tag, &g->cfg) > 0) {
            g->tag.samplerate_in = g->p.samplerate;
            g->tag.music_crc = crc;
            g->tag_placeholder_pending = 1;
        }
    }
    return 0;
}

/* reference lame.h:970, VbrTag.c:900: the final tag frame that replaces the placeholder at the
 * head of the stream; 0 when the tag is off or nothing was encoded; the needed size when `size'
 * is too small */
extern "C" size_t
lame_get_lametag_frame(const lame_t g, unsigned char *buffer, size_t size)
{
    if (!valid(g) || !g->inited || !g->write_vbr_tag)
        return 0;
    g->tag.nogap_total = g->nogap_total;       /* (the frontend sets these per file, after lame_init_params) */
    g->tag.nogap_current = g->nogap_current;
    return (size_t) lh_tag_frame(&g->tag, &g->cfg, g->cfg.vbr_q, g->enc_padding,
                                 g->have_last ? g->last_frame.mode_ext : 0, buffer, (long) size);
}

extern "C" int
lame_close(lame_t g)
{
    LhDeviceScope const on_device(valid(g) ? g->device : -1);
    if (!valid(g))
        return -3;
    g->class_id = 0;
    g->dc.release();
    if (g->bs.buf)
        lh_bs_free(&g->bs);
    free(g->tab);
    free(g->rs);
    free(g->rg);
    delete  g;                  /* (its device memory and its stream go here, on the handle's device) */
    return 0;
}

/* runs the device self-test of the wave primitives; returns the number of
 * mismatches (0 = pass) or a negative error */
extern "C" int
lamehip_selftest(void)
{
    LhDevBuf < unsigned >d;
    unsigned h = 0xffffffffu;
    if (lamehip_device_count() <= 0)
        return LAMEHIP_ERR_NODEVICE;
    HIPCHK(d.alloc(1));
    for (unsigned seed = 1; seed <= 4; seed++) {
        int     rc = lh_launch_selftest(d.get(), seed * 7919u, nullptr);
        if (rc)
            return set_err("selftest launch", (hipError_t) rc);
        HIPCHK(hipMemcpy(&h, d.get(), sizeof(h), hipMemcpyDeviceToHost));
        if (h != 0)
            break;
    }
    return (int) h;
}

/* sizes of the POD layouts this build was compiled with (ABI check for bindings) */
extern "C" int
lamehip_abi_sizeof(int which)
{
    switch (which) {
    case 0:
        return (int) sizeof(LhConfig);
    case 1:
        return (int) sizeof(LhTables);
    case 2:
        return (int) sizeof(LhFrameOut);
    case 3:
        return (int) sizeof(LhGranule);
    case 4:
        return (int) sizeof(LhStreamState);
    case 5:
        return (int) sizeof(LhStreamDesc);
    }
    return -1;
}

extern "C" int
lamehip_get_config(const lame_t g, void *out, int size)
{
    if (!valid(g) || !g->inited || size < (int) sizeof(LhConfig))
        return -1;
    memcpy(out, &g->cfg, sizeof(LhConfig));
    return (int) sizeof(LhConfig);
}

extern "C" int
lamehip_get_tables(const lame_t g, void *out, int size)
{
    if (!valid(g) || !g->inited || !g->tab || size < (int) sizeof(LhTables))
        return -1;
    memcpy(out, g->tab, sizeof(LhTables));
    return (int) sizeof(LhTables);
}

/* the handle's device for its own launches; call before lame_init_params (reference: none -- the
 * reference has no devices; the frontend's handle simply lives on the current device by default) */
extern "C" int
lamehip_set_device(lame_t g, int device)
{
    if (!valid(g) || g->inited || device < 0)
        return -1;
    g->device = device;
    return 0;
}

/* debug aid: raw LhStreamState carried by a single-stream handle between launches */
extern "C" int
lamehip_get_state(const lame_t g, void *out, int size)
{
    LhDeviceScope const on_device(valid(g) ? g->device : -1);
    if (!g || !g->have_device || size < (int) sizeof(LhStreamState))
        return -1;
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(hipMemcpy(out, g->d_state.get(), sizeof(LhStreamState), hipMemcpyDeviceToHost));
    return (int) sizeof(LhStreamState);
}

