/*
 * tag_info_host_check.c -- TEST TOOL: the tag frame of a stream that arrives at an input rate of its own
 * (lamehip_batch_set_stream_in_samplerate with lamehip_batch_set_incremental_tagging), made on the host the way the final
 * step of lh_tag_resume_kernel makes it, as a program of its own under AddressSanitizer and UBSan
 * (tests/hipemu_rs_mixed/Makefile).  The batch has ONE template, made for its own input rate; a stream's info byte -- the
 * source frequency and the "non-optimal" bit, which lh_tag_template makes of the input rate -- travels with the stream's
 * end padding in one entry of the padding table (lh_tag.h: lh_tag_pad_with_info) and takes the template's place before the
 * two CRCs are taken.  For every setting and every stream rate:
 *   - the entry gives back the padding and the byte; an entry without a byte says so;
 *   - template (batch's rate) + the entry's byte + seek table + lh_tag_finish_fields is lh_tag_frame with the stream's
 *     rate as its source rate, whole frame: the info byte and both CRCs among it;
 *   - for the batch's own rate the entry carries no byte and the frame is the template's.
 * Prints "rate <hz> info <byte>" per stream rate of the first setting (tests/test_mixed_rates_plan.py compares them with
 * the reference's lame_get_lametag_frame where the reference is built); exit status 0 = ok.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"

static const int rates[] = { 8000, 32000, 44100, 48000, 96000, 22050, 44110, 32001 };
#define NRATES ((int) (sizeof(rates) / sizeof(rates[0])))

static int
check(int batch_rate, int vbr, int error_protection, int channels, int say)
{
    LhUserParams up;
    LhConfig c;
    LhInitAux aux;
    LhVbrTag v;
    LhTagParams tp;
    unsigned char *tmpl, *made, *want;
    int     total, k, i, f;
    lh_params_default(&up);
    up.samplerate = batch_rate;
    up.samplerate_out = 44100;
    up.channels = channels;
    up.brate = 128;
    up.vbr = vbr;
    up.vbr_q = 2;
    up.error_protection = error_protection;
    if (lh_config_resolve(&up, &c, &aux) != 0)
        return 1;
    total = lh_tag_init(&v, &c);
    if (total <= 0)
        return 2;
    lh_tag_params(&v, &c, &tp);
    for (f = 0; f < 37; f++)
        lh_tag_add_frame(&v, lh_tag_kbps(c.version, c.vbr == 0 ? c.bitrate_index : c.vbr_min_bitrate_index + f % 3));
    v.bytes_written = 15437;
    v.music_crc = 0xBEE5;
    tmpl = (unsigned char *) malloc((size_t) total);
    made = (unsigned char *) malloc((size_t) total);
    want = (unsigned char *) malloc((size_t) total);
    if (!tmpl || !made || !want)
        return 3;
    v.samplerate_in = batch_rate;
    lh_tag_template(&v, &c, c.vbr_q, tmpl);
    for (k = 0; k < NRATES; k++) {
        int const padding = 576 + 97 * k;
        int     entry, info;
        /* the stream's byte, as the batch makes it: out of a template for the stream's rate */
        v.samplerate_in = rates[k];
        lh_tag_template(&v, &c, c.vbr_q, made);
        info = made[tp.at + LH_TAG_AT_EXT + LH_TAG_EXT_INFO];
        entry = rates[k] == batch_rate ? padding : lh_tag_pad_with_info(padding, info);
        if (lh_tag_pad_padding(entry) != padding || lh_tag_pad_info(entry) != (rates[k] == batch_rate ? -1 : info))
            return 4;
        /* the final step: the batch's template, the entry's byte, the seek table, the fields and the CRCs */
        memcpy(made, tmpl, (size_t) total);
        if (lh_tag_pad_info(entry) >= 0)
            made[tp.at + LH_TAG_AT_EXT + LH_TAG_EXT_INFO] = (unsigned char) lh_tag_pad_info(entry);
        for (i = 1; i < 100; i++)
            made[tp.at + LH_TAG_AT_TOC + i] = lh_tag_toc_entry(i, v.bag, v.pos, v.sum);
        lh_tag_finish_fields(made, tp.at, tp.sideinfo_len, tp.error_protection, v.num_frames,
                             (uint32_t) (v.bytes_written + (unsigned long) total), v.music_crc, lh_tag_pad_padding(entry), 2);
        if (lh_tag_frame(&v, &c, c.vbr_q, padding, 2, want, total) != total)
            return 5;
        if (memcmp(made, want, (size_t) total) != 0)
            return 6;
        /* (the bits the input rate decides: source frequency in bits 6..7, non-optimal in bit 5) */
        if ((info >> 6) != (rates[k] <= 32000 ? 0 : rates[k] == 48000 ? 2 : rates[k] > 48000 ? 3 : 1))
            return 7;
        if (rates[k] <= 32000 && !(info & 0x20))
            return 8;
        if (say)
            printf("rate %d info %d\n", rates[k], info);
    }
    free(tmpl);
    free(made);
    free(want);
    return 0;
}

int
main(void)
{
    static const int batch_rates[] = { 48000, 22050, 8000, 96000 };
    int     bad = 0, rc, b, vbr, ep;
    for (b = 0; b < 4; b++)
        for (vbr = 0; vbr <= 4; vbr += 4)
            for (ep = 0; ep < 2; ep++)
                if ((rc = check(batch_rates[b], vbr, ep, 2 - (b + ep) % 2,b == 0 && vbr == 0 && ep == 0)) != 0) {
                    printf("batch at %d Hz, vbr %d, crc %d: FAILED check %d\n", batch_rates[b], vbr, ep, rc);
                    bad++;
                }
    if (!bad)
        printf("ok\n");
    return bad ? 1 : 0;
}
