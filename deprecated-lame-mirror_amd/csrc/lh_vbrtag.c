/*
 * lh_vbrtag.c -- host side: the Xing/"Info" + LAME tag frame of a CBR stream
 * (SURVEY.md 8(f) row 3).  Behaviour of the reference's libmp3lame/VbrTag.c:
 *   - lame_init_params reserves a frame-sized placeholder at the start of the stream
 *     (InitVbrTag :492-581; all zero after the 4 header bytes),
 *   - every encoded frame adds its bit rate to a bounded seek-point bag (AddVbrFrame :196,
 *     addVbr :124-148),
 *   - the audio bytes handed to the caller feed a CRC-16 and a byte count
 *     (bitstream.c:1078-1090),
 *   - lame_get_lametag_frame (:900-1018) builds the final frame: "Info", frame and byte
 *     counts, a 100-entry seek table (Xing_seek_table :151-172) and the LAME extension
 *     (PutLameVBR :615-861) with two CRCs.
 * Everything here is byte bookkeeping on the host; nothing touches the GPU.
 */
#include <math.h>
#include <string.h>
#include "lh_host.h"

typedef char lh_tag_delay_is_the_encoders[LH_TAG_ENCDELAY == LH_ENCDELAY ? 1 : -1];

static uint16_t lh_crc16_tab[256];
static int lh_crc16_ready = 0;

static void
crc16_init(void)
{
    /* CRC-16 with the reflected polynomial 0xA001, the table the reference spells out
     * (VbrTag.c:73-106) */
    int     i, k;
    for (i = 0; i < 256; i++) {
        uint16_t c = (uint16_t) i;
        for (k = 0; k < 8; k++)
            c = (uint16_t) ((c & 1) ? (c >> 1) ^ 0xA001 : (c >> 1));
        lh_crc16_tab[i] = c;
    }
    lh_crc16_ready = 1;
}

static uint16_t
crc16_update(uint16_t value, uint16_t crc)
{
    uint16_t const tmp = (uint16_t) (crc ^ value);
    return (uint16_t) ((crc >> 8) ^ lh_crc16_tab[tmp & 0xff]);
}

void
lh_tag_crc(LhVbrTag * v, const unsigned char *buf, long n)
{
    long    i;
    if (!lh_crc16_ready)
        crc16_init();
    for (i = 0; i < n; i++)
        v->music_crc = crc16_update(buf[i], v->music_crc);
    v->bytes_written += (unsigned long) n;
}

/* kbps of a bitrate index in the stream's MPEG version (what AddVbrFrame accumulates, reference VbrTag.c:195-201) */
int
lh_tag_kbps(int version, int bitrate_index)
{
    return lh_bitrate_row(version)[bitrate_index & 15];
}

/* the bit rate of the tag frame itself (reference VbrTag.c:515-529, 287-300): the stream's own for CBR, else 128 / 64 /
 * 32 kb/s for MPEG-1 / 2 / 2.5, and its index in the version's row (2.5: the MPEG-2 row holds 32 at the same index) */
static int
tag_frame_kbps(const LhConfig * c)
{
    if (c->vbr == 0)
        return c->avg_bitrate;
    return c->version == 1 ? 128 : (c->samplerate < 16000 ? 32 : 64);
}

static int
tag_frame_bitrate_index(const LhConfig * c)
{
    int const kbps = tag_frame_kbps(c);
    int     i;
    if (c->vbr == 0)
        return c->bitrate_index;
    for (i = 1; i <= 14; i++)
        if (lh_bitrate_row(c->version)[i] == kbps)
            return i;
    return 0;
}

/* reference VbrTag.c:492-559: 0 = the tag does not fit, stays off */
int
lh_tag_init(LhVbrTag * v, const LhConfig * c)
{
    /* CBR: the stream's own frame size; VBR: a 128 / 64 / 32 kbps frame (XING_BITRATE1 / 2 / 25, reference VbrTag.c:515-529) */
    int const kbps_header = tag_frame_kbps(c);
    int const total = ((c->version + 1) * 72000 * kbps_header) / c->samplerate;
    int const header_size = c->sideinfo_len + LH_LAMEHEADERSIZE;
    memset(v, 0, sizeof(*v));
    if (!lh_crc16_ready)
        crc16_init();
    if (total < header_size || total > 2880)
        return 0;
    v->total_frame_size = total;
    v->want = 1;
    v->size = LH_TAG_BAG;
    v->enabled = 1;
    v->samplerate_in = c->samplerate;
    return total;
}

/* Seek-point bookkeeping (reference VbrTag.c:124-148): the running sum of the frames' bit rates is
 * sampled every `want' frames into a bag of fixed size; a full bag keeps every second sample and
 * the sampling distance doubles, so the bag always spans the whole stream evenly. */
void
lh_tag_add_frame(LhVbrTag * v, int kbps)
{
    v->num_frames++;
    v->sum += kbps;
    if (++v->seen < v->want)
        return;
    if (v->pos < v->size) {
        v->bag[v->pos++] = v->sum;
        v->seen = 0;
    }
    if (v->pos == v->size) {
        int     keep;
        for (keep = 0; 2 * keep + 1 < v->size; keep++)
            v->bag[keep] = v->bag[2 * keep + 1];
        v->pos /= 2;
        v->want += v->want;
    }
}

/* the 4 header bytes, reference VbrTag.c:257-323 (MPEG-1, CBR: the stream's own bit rate) */
static void
tag_frame_header(const LhConfig * c, int mode_ext, unsigned char *b)
{
    b[0] = 0xff;
    b[1] = (unsigned char) (0xe0 | ((c->samplerate < 16000 ? 0 : 1) << 4) | (c->version << 3) | (1 << 1)
                            | (c->error_protection ? 0 : 1));
    b[1] = (unsigned char) ((b[1] & 0xf1) | (c->version == 1 ? 0x0a : 0x02));
    b[2] = (unsigned char) (((c->samplerate_index << 2) | (c->extension & 1)) & 0x0d);
    /* bitrate field: the CBR rate, or the tag frame's own for VBR streams (reference VbrTag.c:286-303) */
    b[2] = (unsigned char) (b[2] | (16 * tag_frame_bitrate_index(c)));
    b[3] = (unsigned char) ((c->mode << 6) | ((mode_ext & 3) << 4) | ((c->copyright & 1) << 3)
                            | ((c->original & 1) << 2) | (c->emphasis & 3));
}

/* the placeholder that opens the stream; returns its size */
int
lh_tag_placeholder(const LhVbrTag * v, const LhConfig * c, unsigned char *buf)
{
    memset(buf, 0, (size_t) v->total_frame_size);
    tag_frame_header(c, 0, buf);
    return v->total_frame_size;
}

static void
put_i4(unsigned char *b, uint32_t x)
{
    b[0] = (unsigned char) (x >> 24);
    b[1] = (unsigned char) (x >> 16);
    b[2] = (unsigned char) (x >> 8);
    b[3] = (unsigned char) x;
}

static void
put_i2(unsigned char *b, int x)
{
    b[0] = (unsigned char) ((x >> 8) & 0xff);
    b[1] = (unsigned char) (x & 0xff);
}

/* The frame as far as the settings decide it (lh_tag.h): the header with mode extension 0, "Info" / "Xing", the flags, the
 * static fields of the LAME extension -- v's source rate, radio gain and nogap place among them --, everything a stream
 * decides left zero.  Writes v->total_frame_size bytes. */
void
lh_tag_template(const LhVbrTag * v, const LhConfig * c, int vbr_q, unsigned char *buf)
{
    int     n;
    memset(buf, 0, (size_t) v->total_frame_size);
    tag_frame_header(c, 0, buf);
    n = c->sideinfo_len;
    if (c->error_protection)
        n -= 2;
    memcpy(buf + n, c->vbr == 0 ? "Info" : "Xing", 4);   /* reference VbrTag.c:964-977 */
    n += 4;
    put_i4(buf + n, 0x0001 | 0x0002 | 0x0004 | 0x0008);    /* frames, bytes, TOC, quality */
    n += 4 + 4 + 4 + 100;       /* (the counts and the seek table: the stream's) */
    {
        /* LAME extension, reference PutLameVBR */
        unsigned char *p = buf + n;
        int     k = 0;
        int     quality = 100 - 10 * vbr_q - c->quality;
        double const lp = (c->lowpassfreq / 100.0) + .5;
        unsigned char const lowpass = (unsigned char) (lp > 255 ? 255 : lp);
        int const ath_type = c->ATHtype;
        int const safe_joint = (c->use_safe_joint_stereo != 0);
        int     stereo_mode, source_freq, non_optimal = 0;
        if (quality < 0)
            quality = 0;
        switch (c->mode) {
        case LH_MODE_MONO:
            stereo_mode = 0;
            break;
        case LH_MODE_STEREO:
            stereo_mode = 1;
            break;
        case LH_MODE_DUAL:
            stereo_mode = 2;
            break;
        case LH_MODE_JOINT_STEREO:
            stereo_mode = c->force_ms ? 4 : 3;
            break;
        default:
            stereo_mode = 7;
        }
        if (v->samplerate_in <= 32000)
            source_freq = 0;
        else if (v->samplerate_in == 48000)
            source_freq = 2;
        else if (v->samplerate_in > 48000)
            source_freq = 3;
        else
            source_freq = 1;
        /* short_blocks: 2 = dispensed, 3 = forced (lame.h short_block_t) */
        if (c->short_blocks == 3 || c->short_blocks == 2
            || (c->lowpassfreq == -1 && c->highpassfreq == -1) || (c->disable_reservoir && c->avg_bitrate < 320)
            || (c->ath_flags & 3) || ath_type == 0 || v->samplerate_in <= 32000)
            non_optimal = 1;
        put_i4(p + k, (uint32_t) quality);
        k += 4;
        memcpy(p + k, "LAME3.99r", 9);  /* get_lame_tag_encoder_short_version() of 3.99.5 */
        k += 9;
        /* tag revision 0 + method (vbr_type_translator, reference VbrTag.c:646): 1 CBR, 5 vbr_mt, 3 vbr_rh, 2 ABR, 4 vbr_mtrh */
        p[k++] = (unsigned char) (c->vbr == 0 ? 1 : (c->vbr == 1 ? 5 : (c->vbr == 2 ? 3 : (c->vbr == 3 ? 2 : 4))));
        p[k++] = lowpass;
        put_i4(p + k, 0);               /* peak signal amplitude: not measured */
        k += 4;
        put_i2(p + k, (uint16_t) lh_tag_gain_field(v->radio_gain_on, v->radio_gain));   /* radio ReplayGain */
        k += 2;
        put_i2(p + k, 0);               /* audiophile ReplayGain */
        k += 2;
        {
            /* --nogap: more titles follow / came before (reference VbrTag.c:728-735) */
            int const more = (v->nogap_total != -1 && v->nogap_current < v->nogap_total - 1);
            int const prev = (v->nogap_total != -1 && v->nogap_current > 0);
            p[k++] = (unsigned char) (ath_type + (1 << 4) + (safe_joint << 5) + (more << 6) + (prev << 7));
        }
        {
            /* CBR: the bit rate; ABR: the mean; VBR: the lowest allowed one (reference VbrTag.c:679-693) */
            int const abr = (c->vbr == 0) ? c->avg_bitrate : (c->vbr == 3) ? c->vbr_avg_bitrate_kbps
                : lh_bitrate_row(c->version)[c->vbr_min_bitrate_index];
            p[k++] = (unsigned char) (abr >= 255 ? 0xFF : abr);
        }
        k += 3;                         /* (encoder delay and end padding: with the stream's fields) */
        p[k++] = (unsigned char) (c->noise_shaping + (stereo_mode << 2) + (non_optimal << 5) + (source_freq << 6));
        p[k++] = 0;                     /* MP3 gain */
        /* preset: apply_preset(brate) leaves the bit rate here (presets.c:361, lame.c:1045);
         * the VBR path applies V0..V9 = 500 - 10 q (lame.c:983) */
        put_i2(p + k, (c->vbr == 0 || c->vbr == 3) ? c->avg_bitrate : 500 - 10 * c->vbr_q);
    }
}

/* what the tag kernel of a device-packed batch needs besides the template (lh_tag.h) */
void
lh_tag_params(const LhVbrTag * v, const LhConfig * c, LhTagParams * p)
{
    static const long run[LH_TAG_NADV] = { 16, 32, 64, 128, 256, 512, 64 * LH_TAG_PIECE, LH_TAG_ROW - LH_TAG_PIECE };
    int     j, k;
    long    i;
    memset(p, 0, sizeof(*p));
    p->total = v->total_frame_size;
    p->at = c->sideinfo_len - (c->error_protection ? 2 : 0);
    p->sideinfo_len = c->sideinfo_len;
    p->error_protection = c->error_protection != 0;
    for (k = 0; k < 16; k++)
        p->kbps[k] = lh_bitrate_row(c->version)[k];
    for (j = 0; j < LH_TAG_NADV; j++)
        for (k = 0; k < 16; k++) {
            uint32_t crc = 1u << k;
            for (i = 0; i < run[j]; i++)
                crc = lh_tag_crc_byte(crc, 0);
            p->adv[j][k] = (uint16_t) crc;
        }
}

/* The advance matrices of an incremental batch's tag kernel (lh_tag.h: LhTagPow): a byte's step for k = 0, and every
 * further one the one before applied to itself -- a run of 2 << k zeros is a run of 1 << k twice. */
void
lh_tag_pow_table(LhTagPow * t)
{
    int     j, k;
    for (k = 0; k < 16; k++)
        t->col[0][k] = (uint16_t) lh_tag_crc_byte(1u << k, 0);
    for (j = 1; j < LH_TAG_NPOW; j++)
        for (k = 0; k < 16; k++)
            t->col[j][k] = (uint16_t) lh_tag_crc_advance(t->col[j - 1][k], t->col[j - 1]);
}

/* final tag frame; returns the frame size, 0 when there is no tag (reference VbrTag.c:900-1018): the template, finished
 * with the stream's own fields (lh_tag.h).  vbr_q is the caller-level setting the "quality" byte is made of. */
int
lh_tag_frame(const LhVbrTag * v, const LhConfig * c, int vbr_q, int enc_padding, int last_mode_ext,
             unsigned char *buf, long size)
{
    int const at = c->sideinfo_len - (c->error_protection ? 2 : 0);
    uint32_t const music_length = (uint32_t) (v->bytes_written + (unsigned long) v->total_frame_size);
    int     i;
    if (!v->enabled || v->pos <= 0)
        return 0;
    if (size < v->total_frame_size)
        return v->total_frame_size;
    if (!buf)
        return 0;
    lh_tag_template(v, c, vbr_q, buf);
    for (i = 1; i < 100; ++i)
        buf[at + LH_TAG_AT_TOC + i] = lh_tag_toc_entry(i, v->bag, v->pos, v->sum);
    lh_tag_finish_fields(buf, at, c->sideinfo_len, c->error_protection, (uint32_t) v->num_frames, music_length, v->music_crc,
                         enc_padding, last_mode_ext);
    return v->total_frame_size;
}
