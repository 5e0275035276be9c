/*
 * lh_tag.h -- the per-stream half of the Xing/Info + LAME tag frame, ONE text for the host (lh_vbrtag.c, plain C) and
 * the device (lh_tag.hip), and the records the tag kernel of a device-packed batch reads.
 *
 * A tag frame is a TEMPLATE -- everything the settings decide: the header, "Info" / "Xing", the flags, the static fields
 * of the LAME extension; lh_tag_template, host only -- FINISHED with what the stream decides: the last frame's mode
 * extension, the seek table, the frame and byte counts, the end padding, the music CRC and the two CRCs that cover the
 * frame itself (lh_tag_toc_entry, lh_tag_finish_fields).  lh_tag_frame is the one followed by the other; the kernel gets
 * the template from the host once per batch and runs the finish per stream.  lh_tag_patch_gain puts a radio gain into a
 * finished frame that was made without one.
 *
 * The seek table's arithmetic is the reference's (VbrTag.c:151-172): the percent and its product with the bag's fill
 * are float, the scaling to 1/256 is double, and nothing may be fused or reassociated -- the host objects are built with
 * -ffp-contract=off, and the device text names every rounding (LH_TAG_DEVICE).
 */
#ifndef LH_TAG_H
#define LH_TAG_H

#include <stdint.h>
#include <math.h>

#ifndef LH_TAG_FN
#define LH_TAG_FN static inline
#endif

#if defined(LH_TAG_DEVICE) && defined(__HIP_DEVICE_COMPILE__)
#define LH_TAG_FDIV(a, b) __fdiv_rn((a), (b))
#define LH_TAG_FMUL(a, b) __fmul_rn((a), (b))
#define LH_TAG_DMUL(a, b) __dmul_rn((a), (b))
#define LH_TAG_DDIV(a, b) __ddiv_rn((a), (b))
#else
#define LH_TAG_FDIV(a, b) ((a) / (b))
#define LH_TAG_FMUL(a, b) ((a) * (b))
#define LH_TAG_DMUL(a, b) ((a) * (b))
#define LH_TAG_DDIV(a, b) ((a) / (b))
#endif

#define LH_TAG_BAG_SIZE 400     /* LH_TAG_BAG of lh_host.h: seek points the bag holds */
#define LH_TAG_ENCDELAY 576     /* LH_ENCDELAY of lamehip_types.h */
/* places behind `at', where "Info" / "Xing" stands */
#define LH_TAG_AT_FRAMES 8
#define LH_TAG_AT_BYTES 12
#define LH_TAG_AT_TOC 16
#define LH_TAG_AT_EXT 116       /* the LAME extension (reference PutLameVBR) ... */
#define LH_TAG_EXT_GAIN 19      /* ... and in it: the radio ReplayGain field, */
#define LH_TAG_EXT_PADDING 25   /* encoder delay and end padding, 12 bits each, */
#define LH_TAG_EXT_INFO 28      /* the info byte: noise shaping, stereo mode, "non-optimal" and the source frequency, */
#define LH_TAG_EXT_LENGTH 32    /* the music's length, */
#define LH_TAG_EXT_MUSIC_CRC 36 /* its CRC, */
#define LH_TAG_EXT_CRC 38       /* and the CRC of the frame up to here */

/* The tag kernel's workgroup: LH_TAG_NT lanes, one stream; a lane takes LH_TAG_PIECE bytes of every LH_TAG_ROW. */
#define LH_TAG_NT 256
#define LH_TAG_PIECE 16
#define LH_TAG_ROW (LH_TAG_NT * LH_TAG_PIECE)
/* the music CRC moved on over a run of zero bytes, as 16 columns of a bit matrix per run length: 16 << j bytes for
 * j = 0 .. 5 (the fold across a wave's lanes), a wave's 1024 (the fold across the waves), and a row less a piece (a lane's
 * next piece) */
#define LH_TAG_ADV_WAVE 6
#define LH_TAG_ADV_GAP 7
#define LH_TAG_NADV 8

typedef struct LhTagParams {
    int     total;              /* the frame's size (lh_tag_init) */
    int     at;                 /* where "Info" / "Xing" stands */
    int     sideinfo_len;
    int     error_protection;
    int16_t kbps[16];           /* the MPEG version's bit rates by index */
    uint16_t adv[LH_TAG_NADV][16];
} LhTagParams;

/* An incremental batch that packs on the device (lamehip_batch_set_incremental_tagging): what a stream's tag carries from
 * round to round in HBM, all zero at first.  lh_tag_resume_kernel moves it on behind every round's drain: the music CRC
 * over the bytes that are final, the bookkeeping of lh_tag_add_frame over the round's records; behind the flush it makes
 * the frame of it. */
typedef struct LhTagCarry {
    long long crc_upto;         /* bytes of the slice the CRC covers: [0, crc_upto) */
    uint32_t crc;               /* the music CRC over them */
    int     frames;             /* frames seen */
    int     want;               /* the bag's sampling distance (0 counts as 1: no frame yet) */
    int     pos;                /* samples in the bag */
    int     sum;                /* the frames' bit rates added up */
    int     mode_ext;           /* the last frame's */
    int     bad;                /* a round found a status, or a position that does not continue the last one: no tag */
    int     pad;
    int     bag[LH_TAG_BAG_SIZE];
} LhTagCarry;

/* the music CRC moved on over a run of 1 << k zero bytes, k = 0 .. LH_TAG_NPOW - 1, 16 columns each: a run of any length
 * is the runs of its set bits one after the other (lh_tag_crc_advance_by).  Made on the host (lh_tag_pow_table). */
#define LH_TAG_NPOW 40
typedef struct LhTagPow {
    uint16_t col[LH_TAG_NPOW][16];
} LhTagPow;

/* A stream of an incremental batch whose input rate is its own (lamehip_batch_set_stream_in_samplerate) has its own info
 * byte -- the source frequency and the "non-optimal" bit are made of the input rate, lh_tag_template --, which travels with
 * the stream's end padding (12 bits) in the table the final step of lh_tag_resume_kernel reads: bit 24 says there is one,
 * bits 16 .. 23 are the byte.  The step puts it into the template's copy before the frame's CRCs are taken. */
LH_TAG_FN int
lh_tag_pad_with_info(int enc_padding, int info)
{
    return (enc_padding & 0xffff) | ((info & 0xff) << 16) | (1 << 24);
}

LH_TAG_FN int
lh_tag_pad_padding(int entry)
{
    return entry & 0xffff;
}

/* the info byte of a table entry, or -1: the template's */
LH_TAG_FN int
lh_tag_pad_info(int entry)
{
    return ((entry >> 24) & 1) ? ((entry >> 16) & 0xff) : -1;
}

/* one byte into the music CRC (reflected polynomial 0xA001, reference VbrTag.c:73-122) without a table: the byte's eight
 * steps shift its bits out through taps 0, 13 and 15 -- each bit lands 6 and 7 places up, and their parity on both ends */
LH_TAG_FN uint32_t
lh_tag_crc_byte(uint32_t crc, uint32_t byte)
{
    uint32_t const d = (crc ^ byte) & 0xffu;
    uint32_t const par = (uint32_t) __builtin_popcount(d) & 1u;
    return (crc >> 8) ^ (d << 6) ^ (d << 7) ^ (par * 0xC001u);
}

/* the CRC moved on over the run of zero bytes `col' stands for */
LH_TAG_FN uint32_t
lh_tag_crc_advance(uint32_t crc, const uint16_t *col)
{
    uint32_t out = 0;
    int     k;
    for (k = 0; k < 16; k++)
        out ^= (0u - ((crc >> k) & 1u)) & col[k];
    return out;
}

/* ... over a run of n zero bytes, n >= 0: through the set bits of n */
LH_TAG_FN uint32_t
lh_tag_crc_advance_by(uint32_t crc, const LhTagPow * t, long long n)
{
    int     k;
    for (k = 0; k < LH_TAG_NPOW && (n >> k) != 0; k++)
        if ((n >> k) & 1)
            crc = lh_tag_crc_advance(crc, t->col[k]);
    return crc;
}

/* the bag's sampling distance after n frames: the smallest power of two with n / want < LH_TAG_BAG_SIZE */
LH_TAG_FN int
lh_tag_want(int n)
{
    int     w = 1;
    while (n / w >= LH_TAG_BAG_SIZE)
        w += w;
    return w;
}

/* CRC-16 of a frame's protected part (lh_header_crc of lh_bitstream.c, which the host packer keeps for itself) */
LH_TAG_FN unsigned
lh_tag_header_crc(const unsigned char *h, int len)
{
    unsigned crc = 0xffffu;
    int     i, b;
    for (i = 2; i < len; i++) {
        if (i == 4 || i == 5)
            continue;
        for (b = 7; b >= 0; b--) {
            unsigned const in = (h[i] >> b) & 1u, top = (crc >> 15) & 1u;
            crc = (crc << 1) & 0xffffu;
            if (in ^ top)
                crc ^= 0x8005u;
        }
    }
    return crc;
}

/* the radio ReplayGain field (reference VbrTag.c:704-721): name code 1, originator "automatic", sign, |gain| in tenths of
 * a dB; all zero when it was not measured */
LH_TAG_FN unsigned
lh_tag_gain_field(int on, int rg)
{
    if (!on)
        return 0;
    rg = rg > 0x1FE ? 0x1FE : (rg < -0x1FE ? -0x1FE : rg);
    return 0x2000u | 0xC00u | (rg >= 0 ? (unsigned) rg : (0x200u | (unsigned) -rg));
}

/* entry i (1 .. 99) of the seek table: where i percent of the playing time lies, in 1/256 of the byte count -- the bag
 * sample nearest below, relative to the final sum (float index and ratio, double scaling, as the reference's
 * Xing_seek_table evaluates them) */
LH_TAG_FN unsigned char
lh_tag_toc_entry(int i, const int *bag, int pos, int sum)
{
    float const percent = LH_TAG_FDIV((float) i, (float) 100);
    int     slot = (int) (floor((double) LH_TAG_FMUL(percent, (float) pos))), where;
    float   upto, all;
    slot = slot > pos - 1 ? pos - 1 : slot;
    upto = (float) bag[slot];
    all = (float) sum;
    where = (int) LH_TAG_DDIV(LH_TAG_DMUL(256., (double) upto), (double) all);
    return (unsigned char) (where > 255 ? 255 : where);
}

/* everything else a stream decides, into a template whose seek table is in place; music_length counts the tag frame */
LH_TAG_FN void
lh_tag_finish_fields(unsigned char *buf, int at, int sideinfo_len, int error_protection, uint32_t num_frames, uint32_t music_length,
                     uint32_t music_crc, int enc_padding, int last_mode_ext)
{
    unsigned char *const p = buf + at + LH_TAG_AT_EXT;
    uint32_t crc = 0;
    int     i;
    buf[3] = (unsigned char) (buf[3] | ((last_mode_ext & 3) << 4));
    buf[at + LH_TAG_AT_FRAMES] = (unsigned char) (num_frames >> 24);
    buf[at + LH_TAG_AT_FRAMES + 1] = (unsigned char) (num_frames >> 16);
    buf[at + LH_TAG_AT_FRAMES + 2] = (unsigned char) (num_frames >> 8);
    buf[at + LH_TAG_AT_FRAMES + 3] = (unsigned char) num_frames;
    buf[at + LH_TAG_AT_BYTES] = (unsigned char) (music_length >> 24);
    buf[at + LH_TAG_AT_BYTES + 1] = (unsigned char) (music_length >> 16);
    buf[at + LH_TAG_AT_BYTES + 2] = (unsigned char) (music_length >> 8);
    buf[at + LH_TAG_AT_BYTES + 3] = (unsigned char) music_length;
    if (error_protection) {
        /* the tag frame carries a header CRC like any other frame (reference VbrTag.c:996-999); it covers the first bytes
         * of the tag, which start two bytes early in this case */
        unsigned const hc = lh_tag_header_crc(buf, sideinfo_len);
        buf[4] = (unsigned char) (hc >> 8);
        buf[5] = (unsigned char) (hc & 255u);
    }
    p[LH_TAG_EXT_PADDING] = (unsigned char) (LH_TAG_ENCDELAY >> 4);
    p[LH_TAG_EXT_PADDING + 1] = (unsigned char) ((LH_TAG_ENCDELAY << 4) + (enc_padding >> 8));
    p[LH_TAG_EXT_PADDING + 2] = (unsigned char) enc_padding;
    p[LH_TAG_EXT_LENGTH] = (unsigned char) (music_length >> 24);
    p[LH_TAG_EXT_LENGTH + 1] = (unsigned char) (music_length >> 16);
    p[LH_TAG_EXT_LENGTH + 2] = (unsigned char) (music_length >> 8);
    p[LH_TAG_EXT_LENGTH + 3] = (unsigned char) music_length;
    p[LH_TAG_EXT_MUSIC_CRC] = (unsigned char) ((music_crc >> 8) & 0xffu);
    p[LH_TAG_EXT_MUSIC_CRC + 1] = (unsigned char) (music_crc & 0xffu);
    for (i = 0; i < at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC; i++)
        crc = lh_tag_crc_byte(crc, buf[i]);
    p[LH_TAG_EXT_CRC] = (unsigned char) ((crc >> 8) & 0xffu);
    p[LH_TAG_EXT_CRC + 1] = (unsigned char) (crc & 0xffu);
}

/* a finished frame made without a radio gain gets one: the field, and the frame's own CRC over it again */
LH_TAG_FN void
lh_tag_patch_gain(unsigned char *buf, int at, int radio_gain)
{
    unsigned char *const p = buf + at + LH_TAG_AT_EXT;
    unsigned const field = lh_tag_gain_field(1, radio_gain);
    uint32_t crc = 0;
    int     i;
    p[LH_TAG_EXT_GAIN] = (unsigned char) ((field >> 8) & 0xffu);
    p[LH_TAG_EXT_GAIN + 1] = (unsigned char) (field & 0xffu);
    for (i = 0; i < at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC; i++)
        crc = lh_tag_crc_byte(crc, buf[i]);
    p[LH_TAG_EXT_CRC] = (unsigned char) ((crc >> 8) & 0xffu);
    p[LH_TAG_EXT_CRC + 1] = (unsigned char) (crc & 0xffu);
}

#endif
