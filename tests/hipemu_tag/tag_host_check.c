/*
 * tag_host_check.c -- TEST TOOL: the host side of the tag frames of a device-packed batch (lh_tag_template, lh_tag_params,
 * lh_tag.h's finish and gain patch, lh_tag_frame on top of them) run as a program of its own over a list of settings, built
 * with AddressSanitizer and UBSan (tests/hipemu_tag/Makefile).  It checks what needs no reference: the frame fills its
 * buffer and no more; the frame's own CRC, made without a table, is the one the table CRC (lh_tag_crc) makes of the same
 * bytes; the template finished by hand is lh_tag_frame's frame; a frame made without a gain and patched is the frame made
 * with that gain; the kernel's advance matrices move a CRC over zeros as the table CRC does, and fold two CRCs into that
 * of the joined bytes.  Prints one line per case; exit status 0 = ok.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"

static unsigned rnd_state = 12345u;

static unsigned
rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

static unsigned
table_crc(const unsigned char *buf, long n)
{
    LhVbrTag t;
    memset(&t, 0, sizeof(t));
    lh_tag_crc(&t, buf, n);
    return t.music_crc;
}

typedef struct Case {
    const char *name;
    int     samplerate, brate, vbr, vbr_q, abr, channels, error_protection;
} Case;

static int
check(const Case * k, int nframes)
{
    LhUserParams up;
    LhConfig c;
    LhInitAux aux;
    LhVbrTag v;
    LhTagParams tp;
    unsigned char *frame, *byhand, *plain;
    int     total, f, i, at;
    static const int gains[6] = { -0x1FF, -1, 0, 1, 64, 0x1FF };
    lh_params_default(&up);
    up.samplerate = k->samplerate;
    up.channels = k->channels;
    up.brate = k->brate;
    up.vbr = k->vbr;
    up.vbr_q = k->vbr_q;
    up.abr_kbps = k->abr;
    up.error_protection = k->error_protection;
    if (lh_config_resolve(&up, &c, &aux) != 0)
        return 1;
    total = lh_tag_init(&v, &c);
    if (total <= 0)
        return 2;
    for (f = 0; f < nframes; f++) {
        int const lo = c.vbr == 0 ? c.bitrate_index : c.vbr_min_bitrate_index, hi = c.vbr == 0 ? c.bitrate_index : c.vbr_max_bitrate_index;
        lh_tag_add_frame(&v, lh_tag_kbps(c.version, lo + (int) (rnd() % (unsigned) (hi - lo + 1))));
    }
    v.bytes_written = 417ul * (unsigned long) nframes + rnd() % 400u;
    v.music_crc = (uint16_t) rnd();
    /* exactly `total' bytes each: a byte beyond is the sanitizer's */
    frame = (unsigned char *) malloc((size_t) total);
    byhand = (unsigned char *) malloc((size_t) total);
    plain = (unsigned char *) malloc((size_t) total);
    if (!frame || !byhand || !plain)
        return 3;
    memset(frame, 0xA5, (size_t) total);
    if (lh_tag_frame(&v, &c, c.vbr_q, 1105, 2, frame, total) != (nframes > 0 ? total : 0))
        return 4;
    if (nframes == 0) {
        for (i = 0; i < total; i++)
            if (frame[i] != 0xA5)
                return 5;       /* no frames: no tag, the buffer is left alone */
        free(frame);
        free(byhand);
        free(plain);
        printf("%-28s %4d frames: no tag\n", k->name, nframes);
        return 0;
    }
    lh_tag_params(&v, &c, &tp);
    at = tp.at;
    if (tp.total != total || at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC + 2 > total)
        return 6;
    if (memcmp(frame + at, c.vbr == 0 ? "Info" : "Xing", 4) != 0)
        return 7;
    /* the frame's own CRC against the table's */
    if (table_crc(frame, at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC)
        != (unsigned) (frame[at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC] << 8 | frame[at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC + 1]))
        return 8;
    /* the two halves by hand */
    lh_tag_template(&v, &c, c.vbr_q, byhand);
    for (i = 1; i < 100; i++)
        byhand[at + LH_TAG_AT_TOC + i] = lh_tag_toc_entry(i, v.bag, v.pos, v.sum);
    lh_tag_finish_fields(byhand, at, tp.sideinfo_len, tp.error_protection, v.num_frames, (uint32_t) (v.bytes_written + (unsigned long) total),
                         v.music_crc, 1105, 2);
    if (memcmp(byhand, frame, (size_t) total) != 0)
        return 9;
    /* the gain patch */
    for (i = 0; i < 6; i++) {
        v.radio_gain_on = 0;
        if (lh_tag_frame(&v, &c, c.vbr_q, 1105, 2, plain, total) != total)
            return 10;
        lh_tag_patch_gain(plain, at, gains[i]);
        v.radio_gain_on = 1;
        v.radio_gain = gains[i];
        if (lh_tag_frame(&v, &c, c.vbr_q, 1105, 2, byhand, total) != total)
            return 11;
        if (memcmp(plain, byhand, (size_t) total) != 0)
            return 12;
    }
    printf("%-28s %4d frames: %d bytes, tag at %d, crc %02x%02x\n", k->name, nframes, total, at,
           frame[at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC], frame[at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC + 1]);
    free(frame);
    free(byhand);
    free(plain);
    return 0;
}

/* the advance matrices of lh_tag_params against the table CRC */
static int
check_advance(void)
{
    static const long run[LH_TAG_NADV] = { 16, 32, 64, 128, 256, 512, 1024, LH_TAG_ROW - LH_TAG_PIECE };
    LhUserParams up;
    LhConfig c;
    LhInitAux aux;
    LhVbrTag v;
    LhTagParams tp;
    int     j;
    long    i;
    lh_params_default(&up);
    up.samplerate = 44100;
    up.channels = 2;
    up.brate = 128;
    if (lh_config_resolve(&up, &c, &aux) != 0 || lh_tag_init(&v, &c) <= 0)
        return 1;
    lh_tag_params(&v, &c, &tp);
    for (j = 0; j < LH_TAG_NADV; j++) {
        long const na = 1 + (long) (rnd() % 300u), nb = run[j];
        unsigned char *ab = (unsigned char *) calloc((size_t) (na + nb), 1);
        unsigned ca, cb, cz;
        if (!ab)
            return 2;
        for (i = 0; i < na; i++)
            ab[i] = (unsigned char) rnd();
        ca = table_crc(ab, na);
        cz = table_crc(ab, na + nb);    /* (the run still zeros) */
        if (lh_tag_crc_advance(ca, tp.adv[j]) != cz)
            return 3;
        for (i = 0; i < nb; i++)
            ab[na + i] = (unsigned char) rnd();
        cb = table_crc(ab + na, nb);
        if ((lh_tag_crc_advance(ca, tp.adv[j]) ^ cb) != table_crc(ab, na + nb))
            return 4;
        free(ab);
    }
    printf("advance matrices: %d run lengths ok\n", LH_TAG_NADV);
    return 0;
}

int
main(void)
{
    static const Case cases[] = {
        {"CBR 128 at 48 kHz", 48000, 128, 0, 4, 128, 2, 0}, {"CBR 320 at 48 kHz", 48000, 320, 0, 4, 128, 2, 0},
        {"-V2", 44100, 128, 4, 2, 128, 2, 0}, {"ABR 150", 44100, 128, 3, 4, 150, 2, 0},
        {"--vbr-old -V3", 44100, 128, 2, 3, 128, 2, 0}, {"CBR 64 at 22.05 kHz", 22050, 64, 0, 4, 128, 2, 0},
        {"CBR 32 at 12 kHz", 12000, 32, 0, 4, 128, 2, 0}, {"CBR 128 mono", 44100, 128, 0, 4, 128, 1, 0},
        {"CBR 160 error protection", 44100, 160, 0, 4, 128, 2, 1}, {"-V4 error protection", 44100, 128, 4, 4, 128, 2, 1},
    };
    static const int counts[] = { 0, 1, 2, 399, 400, 401, 799, 800, 801, 1700 };
    size_t  k, n;
    int     bad = 0;
    for (k = 0; k < sizeof(cases) / sizeof(cases[0]); k++)
        for (n = 0; n < sizeof(counts) / sizeof(counts[0]); n++) {
            int const rc = check(&cases[k], counts[n]);
            if (rc) {
                printf("%-28s %4d frames: FAILED check %d\n", cases[k].name, counts[n], rc);
                bad++;
            }
        }
    {
        int const rc = check_advance();
        if (rc) {
            printf("advance matrices: FAILED check %d\n", rc);
            bad++;
        }
    }
    return bad ? 1 : 0;
}
