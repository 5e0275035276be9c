/*
 * tag_inc_host_check.c -- TEST TOOL: the host side of the tag frames of an incremental batch that packs on the device
 * (lamehip_batch_set_incremental_tagging) run as a program of its own, built with AddressSanitizer and UBSan
 * (tests/hipemu_tag_inc/Makefile).  It checks what needs no reference and no device:
 *   - the table of advances by powers of two (lh_tag_pow_table): every k up to 20 against lh_tag_crc_byte stepped over
 *     1 << k zeros, every larger one against the one before applied twice, and runs of any length against the table CRC;
 *   - a CRC carried over rounds of any lengths -- the carried one moved on, the new bytes' from 0 XORed in -- is the table
 *     CRC of the prefix;
 *   - the end padding the final round is given completes the stream's frames, for every sample count of a few frames;
 *   - a frame made of a carry -- the bag kept at the sampling distance of the frames so far, thinned out when that grows,
 *     in rounds of any size (lh_tag.h: LhTagCarry, lh_tag_want) -- is lh_tag_frame's, and patched with a gain it is
 *     lh_tag_frame's with that gain.
 * Prints one line per case; exit status 0 = ok.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"

static unsigned rnd_state = 4711u;

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

static int
check_table(void)
{
    LhTagPow *t = (LhTagPow *) malloc(sizeof(LhTagPow));        /* (exactly its size: a column beyond is the sanitizer's) */
    int     j, k, n;
    long    i;
    if (!t)
        return 1;
    lh_tag_pow_table(t);
    for (j = 0; j < LH_TAG_NPOW; j++)
        for (k = 0; k < 16; k++) {
            uint32_t crc = 1u << k;
            if (j <= 20)
                for (i = 0; i < (1l << j); i++)
                    crc = lh_tag_crc_byte(crc, 0);
            else
                crc = lh_tag_crc_advance(lh_tag_crc_advance(crc, t->col[j - 1]), t->col[j - 1]);
            if (t->col[j][k] != crc)
                return 2;
        }
    for (n = 0; n < 40; n++) {
        long const na = 1 + (long) (rnd() % 300u), nz = n < 8 ? n : (long) (rnd() % 300000u);
        unsigned char *ab = (unsigned char *) calloc((size_t) (na + nz), 1);
        if (!ab)
            return 3;
        for (i = 0; i < na; i++)
            ab[i] = (unsigned char) rnd();
        if (lh_tag_crc_advance_by(table_crc(ab, na), t, nz) != table_crc(ab, na + nz))
            return 4;
        free(ab);
    }
    /* (a run longer than any slice: the bits beyond the table are not looked at, the ones inside are) */
    if (lh_tag_crc_advance_by(0x1234u, t, (1ll << 33) + 5) != lh_tag_crc_advance(lh_tag_crc_advance_by(0x1234u, t, 5), t->col[33])
        || lh_tag_crc_advance_by(0x1234u, t, (1ll << 45) + 5) != lh_tag_crc_advance_by(0x1234u, t, 5))
        return 5;
    free(t);
    printf("advance table: %d powers of two ok\n", LH_TAG_NPOW);
    return 0;
}

static int
check_carried_crc(void)
{
    static const long cuts[] = { 0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8193 };
    LhTagPow t;
    int     run, r;
    lh_tag_pow_table(&t);
    for (run = 0; run < 6; run++) {
        long    total = 0, at = 0, i;
        long    plan[13];
        unsigned char *buf;
        uint32_t carried = 0;
        for (r = 0; r < 13; r++) {
            plan[r] = cuts[(r * (run + 1) + run) % 13];
            total += plan[r];
        }
        buf = (unsigned char *) malloc((size_t) total);
        if (!buf)
            return 1;
        for (i = 0; i < total; i++)
            buf[i] = (unsigned char) rnd();
        for (r = 0; r < 13; r++) {
            carried = lh_tag_crc_advance_by(carried, &t, plan[r]) ^ table_crc(buf + at, plan[r]);
            at += plan[r];
            if (carried != table_crc(buf, at))
                return 2;
        }
        free(buf);
    }
    printf("carried CRC: 6 orders of 13 round lengths ok\n");
    return 0;
}

static int
check_padding(void)
{
    static const int fss[2] = { 1152, 576 };
    int     k;
    long    n;
    for (k = 0; k < 2; k++)
        for (n = 0; n < 6 * 1152; n++) {
            int const fs = fss[k], pad = lh_end_padding_fs(n, fs);
            if (pad < 576 || pad >= 576 + fs || pad > 0xfff)
                return 1;       /* (the field has 12 bits) */
            if ((LH_ENCDELAY + n + pad) % fs != 0)
                return 2;
            if (n > 0 && (long) lh_total_frames_fs(n, fs) * fs != LH_ENCDELAY + n + pad)
                return 3;
        }
    printf("end padding: every count up to six frames ok\n");
    return 0;
}

/* one round of a stream's carry: nf frames of the given bit rates (kernel part B, one frame at a time) */
static void
carry_round(LhTagCarry * c, const int *kbps, int nf)
{
    int const want0 = c->want > 0 ? c->want : 1, n1 = c->frames + nf, want1 = lh_tag_want(n1);
    int const step = want1 / want0, keep = c->pos / step;
    int     j, f;
    for (j = 0; j < keep; j++)
        c->bag[j] = c->bag[(j + 1) * step - 1];
    for (f = 0; f < nf; f++) {
        int const g = c->frames + f;
        c->sum += kbps[f];
        if ((g + 1) % want1 == 0)
            c->bag[(g + 1) / want1 - 1] = c->sum;
    }
    c->frames = n1;
    c->want = want1;
    c->pos = n1 / want1;
}

static int
check_carried_frame(int vbr, int error_protection, const int *plan, int nrounds)
{
    LhUserParams up;
    LhConfig c;
    LhInitAux aux;
    LhVbrTag v;
    LhTagParams tp;
    LhTagCarry *carry = (LhTagCarry *) calloc(1, sizeof(LhTagCarry));
    unsigned char *frame, *made;
    int     total, r, f, i, frames = 0;
    static const int gains[4] = { -0x1FF, -7, 0, 64 };
    lh_params_default(&up);
    up.samplerate = 44100;
    up.channels = 2;
    up.brate = 128;
    up.vbr = vbr;
    up.vbr_q = 4;
    up.error_protection = error_protection;
    if (!carry || lh_config_resolve(&up, &c, &aux) != 0)
        return 1;
    total = lh_tag_init(&v, &c);
    if (total <= 0)
        return 2;
    lh_tag_params(&v, &c, &tp);
    for (r = 0; r < nrounds; r++) {
        int    *kbps = (int *) malloc((size_t) (plan[r] > 0 ? plan[r] : 1) * sizeof(int));
        int const lo = c.vbr == 0 ? c.bitrate_index : c.vbr_min_bitrate_index, hi = c.vbr == 0 ? c.bitrate_index : c.vbr_max_bitrate_index;
        if (!kbps)
            return 3;
        for (f = 0; f < plan[r]; f++) {
            kbps[f] = lh_tag_kbps(c.version, lo + (int) (rnd() % (unsigned) (hi - lo + 1)));
            lh_tag_add_frame(&v, kbps[f]);
        }
        carry_round(carry, kbps, plan[r]);
        free(kbps);
        frames += plan[r];
        if (carry->pos != v.pos || carry->want != v.want || carry->sum != v.sum || (unsigned) carry->frames != v.num_frames)
            return 4;
        if (memcmp(carry->bag, v.bag, (size_t) v.pos * sizeof(int)) != 0)
            return 5;
    }
    v.bytes_written = 417ul * (unsigned long) frames + rnd() % 400u;
    v.music_crc = (uint16_t) rnd();
    frame = (unsigned char *) malloc((size_t) total);
    made = (unsigned char *) malloc((size_t) total);
    if (!frame || !made)
        return 6;
    if (lh_tag_frame(&v, &c, c.vbr_q, 1105, 2, frame, total) != total)
        return 7;
    lh_tag_template(&v, &c, c.vbr_q, made);
    for (i = 1; i < 100; i++)
        made[tp.at + LH_TAG_AT_TOC + i] = lh_tag_toc_entry(i, carry->bag, carry->pos, carry->sum);
    lh_tag_finish_fields(made, tp.at, tp.sideinfo_len, tp.error_protection, (uint32_t) carry->frames,
                         (uint32_t) (v.bytes_written + (unsigned long) total), v.music_crc, 1105, 2);
    if (memcmp(made, frame, (size_t) total) != 0)
        return 8;
    for (i = 0; i < 4; i++) {
        unsigned char *patched = (unsigned char *) malloc((size_t) total);
        if (!patched)
            return 9;
        memcpy(patched, made, (size_t) total);
        lh_tag_patch_gain(patched, tp.at, gains[i]);
        v.radio_gain_on = 1;
        v.radio_gain = gains[i];
        if (lh_tag_frame(&v, &c, c.vbr_q, 1105, 2, frame, total) != total || memcmp(patched, frame, (size_t) total) != 0)
            return 10;
        free(patched);
    }
    printf("carried frame (vbr %d, crc %d): %d frames in %d rounds ok\n", vbr, error_protection, frames, nrounds);
    free(frame);
    free(made);
    free(carry);
    return 0;
}

int
main(void)
{
    static const int plan_a[] = { 0, 1, 255, 256, 257, 31, 0, 300, 500, 150 };  /* 512: over 400 in a round; 800 and 1600 at a round's end */
    static const int plan_b[] = { 399, 1, 1, 500, 800 };        /* 400 at a round's end; over 800 and over 1600 in a round */
    static const int plan_c[] = { 1, 1700 };    /* two halvings at once */
    static const int plan_d[] = { 1701 };
    int     bad = 0, rc;
    if ((rc = check_table()) != 0) {
        printf("advance table: FAILED check %d\n", rc);
        bad++;
    }
    if ((rc = check_carried_crc()) != 0) {
        printf("carried CRC: FAILED check %d\n", rc);
        bad++;
    }
    if ((rc = check_padding()) != 0) {
        printf("end padding: FAILED check %d\n", rc);
        bad++;
    }
    if ((rc = check_carried_frame(0, 0, plan_a, 10)) != 0 || (rc = check_carried_frame(4, 0, plan_a, 10)) != 0
        || (rc = check_carried_frame(4, 1, plan_b, 5)) != 0 || (rc = check_carried_frame(4, 0, plan_c, 2)) != 0
        || (rc = check_carried_frame(0, 1, plan_d, 1)) != 0) {
        printf("carried frame: FAILED check %d\n", rc);
        bad++;
    }
    if (!bad)
        printf("ok\n");
    return bad ? 1 : 0;
}
