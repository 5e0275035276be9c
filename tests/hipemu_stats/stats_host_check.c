/*
 * stats_host_check.c -- TEST TOOL: the host text of a batch's statistics (csrc/lh_stats.h, the rule the handle API, the
 * kernel and its host twin count by) run as a program of its own, built with AddressSanitizer and UBSan
 * (tests/hipemu_stats/Makefile).  It checks what needs no reference and no device:
 *   - records that exist exactly -- a heap block of n records with nothing behind it -- are counted without a byte read
 *     outside them, and a carry of exactly its size is written inside it only;
 *   - random records, counted by lh_stats_count_frame, give the tables a plain restatement of the rule gives, for one and
 *     two channels and one and two granules; the granules and channels the stream does not have, filled with 0xA5, change
 *     nothing (and are not read: the rule's answer does not depend on them);
 *   - every bit rate index 0 .. 15 (as a signed byte too), every mode extension, every block type and the mixed flag land in
 *     their bins, and the "all" row and the frame / granule columns are the sums of the others;
 *   - the key of a frame (lh_stats_key) holds LH_STATS_NONE exactly where the stream has no granule or channel.
 * Prints one line per case; exit status 0 = ok.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lh_stats.h"

static unsigned rnd_state = 90210u;

static unsigned
rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

/* the rule once more, written from the reference's updateStats and not from lh_stats.h */
static void
restate(int mode[16][5], int block[16][6], const LhFrameOut * fo, int channels, int mode_gr)
{
    int const bi = fo->bitrate_index & 15, me = fo->mode_ext & 3;
    int     gr, ch;
    mode[bi][4]++;
    mode[15][4]++;
    if (channels == 2) {
        mode[bi][me]++;
        mode[15][me]++;
    }
    for (gr = 0; gr < mode_gr; gr++)
        for (ch = 0; ch < channels; ch++) {
            int     bt = fo->gr[gr][ch].block_type & 3;
            if (fo->gr[gr][ch].mixed_block_flag)
                bt = 4;
            block[bi][bt]++;
            block[bi][5]++;
            block[15][bt]++;
            block[15][5]++;
        }
}

static void
random_record(LhFrameOut * fo, int all_indices)
{
    int     gr, ch;
    memset(fo, 0, sizeof(*fo));
    fo->bitrate_index = (int8_t) (all_indices ? (int) (rnd() % 256u) - 128 : 1 + (int) (rnd() % 14u));
    fo->mode_ext = (int8_t) (rnd() % 4u);
    for (gr = 0; gr < 2; gr++)
        for (ch = 0; ch < 2; ch++) {
            fo->gr[gr][ch].block_type = (int8_t) (rnd() % 4u);
            fo->gr[gr][ch].mixed_block_flag = (int8_t) (rnd() % 7u == 0 && fo->gr[gr][ch].block_type == 2);
        }
}

static int
check_random(int channels, int mode_gr, int n, int all_indices)
{
    LhFrameOut *fr = (LhFrameOut *) malloc((size_t) n * sizeof(LhFrameOut));    /* (exactly n: a record beyond is the sanitizer's) */
    LhStatCarry *c = (LhStatCarry *) calloc(1, sizeof(LhStatCarry)), *c2 = (LhStatCarry *) calloc(1, sizeof(LhStatCarry));
    int     mode[16][5], block[16][6], f, gr, ch, rc = 0;
    if (!fr || !c || !c2)
        return 1;
    memset(mode, 0, sizeof(mode));
    memset(block, 0, sizeof(block));
    for (f = 0; f < n; f++) {
        random_record(&fr[f], all_indices);
        lh_stats_count_frame(c, &fr[f], channels, mode_gr);
        restate(mode, block, &fr[f], channels, mode_gr);
    }
    if (memcmp(c->mode, mode, sizeof(mode)) != 0 || memcmp(c->block, block, sizeof(block)) != 0)
        rc = 2;
    /* what the stream does not have, filled with garbage */
    for (f = 0; f < n; f++) {
        for (gr = 0; gr < 2; gr++)
            for (ch = 0; ch < 2; ch++)
                if (gr >= mode_gr || ch >= channels)
                    memset(&fr[f].gr[gr][ch], 0xA5, sizeof(LhGranule));
        lh_stats_count_frame(c2, &fr[f], channels, mode_gr);
    }
    if (!rc && memcmp(c, c2, sizeof(*c)) != 0)
        rc = 3;
    /* the sums */
    if (!rc) {
        int     row, col, frames = 0, granules = 0;
        for (row = 0; row < 15; row++) {
            int     in_row = 0;
            frames += c->mode[row][4];
            granules += c->block[row][5];
            for (col = 0; col < 5; col++)
                in_row += c->block[row][col];
            if (in_row != c->block[row][5] || c->block[row][5] != c->mode[row][4] * channels * mode_gr)
                rc = 4;
        }
        /* (an index of 15 counts into the "all" row twice, as in the reference's tables) */
        if (!all_indices && (frames != n || c->mode[15][4] != n || granules != n * channels * mode_gr || c->block[15][5] != granules))
            rc = 5;
        if (channels == 1)
            for (row = 0; row < 16; row++)
                for (col = 0; col < 4; col++)
                    if (c->mode[row][col] != 0)
                        rc = 6;
    }
    free(fr);
    free(c);
    free(c2);
    return rc;
}

static int
check_bins(void)
{
    int     bi, me, bt, mixed, rc = 0;
    for (bi = 0; bi < 16 && !rc; bi++)
        for (me = 0; me < 4 && !rc; me++)
            for (bt = 0; bt < 4 && !rc; bt++)
                for (mixed = 0; mixed < 2 && !rc; mixed++) {
                    LhFrameOut *fo = (LhFrameOut *) calloc(1, sizeof(LhFrameOut));
                    LhStatCarry *c = (LhStatCarry *) calloc(1, sizeof(LhStatCarry));
                    int const bin = mixed ? 4 : bt;
                    uint32_t key;
                    if (!fo || !c)
                        return 1;
                    fo->bitrate_index = (int8_t) bi;
                    fo->mode_ext = (int8_t) me;
                    fo->gr[0][0].block_type = (int8_t) bt;
                    fo->gr[0][0].mixed_block_flag = (int8_t) mixed;
                    fo->gr[1][1].block_type = 1;        /* (not the stream's: one granule, one channel) */
                    key = lh_stats_key(fo, 1, 1);
                    if ((key & 15u) != (uint32_t) bi || ((key >> 4) & 3u) != (uint32_t) me || ((key >> 6) & 7u) != (uint32_t) bin
                        || ((key >> 9) & 7u) != LH_STATS_NONE || ((key >> 12) & 7u) != LH_STATS_NONE || ((key >> 15) & 7u) != LH_STATS_NONE)
                        rc = 7;
                    lh_stats_count_frame(c, fo, 1, 1);
                    if (c->block[bi][bin] != (bi == 15 ? 2 : 1) || c->block[15][bin] != (bi == 15 ? 2 : 1) || c->block[15][1] != (bin == 1 ? (bi == 15 ? 2 : 1) : 0)
                        || c->mode[bi][4] != (bi == 15 ? 2 : 1) || c->mode[bi][me] != (me == 4 ? 1 : 0))
                        rc = 8;
                    lh_stats_count_frame(c, fo, 2, 2);
                    if (c->mode[15][me] != (bi == 15 ? 2 : 1) || c->block[15][5] != (bi == 15 ? 10 : 5))
                        rc = 9;
                    free(fo);
                    free(c);
                }
    return rc;
}

int
main(void)
{
    int     channels, mode_gr, rc, bad = 0;
    if (sizeof(LhStatCarry) != LH_STATS_WORDS * sizeof(int)) {
        printf("LhStatCarry is %zu bytes\n", sizeof(LhStatCarry));
        return 1;
    }
    for (channels = 1; channels <= 2; channels++)
        for (mode_gr = 1; mode_gr <= 2; mode_gr++) {
            rc = check_random(channels, mode_gr, 777, 0);
            printf("random records, %d channel(s), %d granule(s): %s (%d)\n", channels, mode_gr, rc ? "FAILED" : "ok", rc);
            bad |= rc;
            rc = check_random(channels, mode_gr, 1, 0);
            printf("one record, %d channel(s), %d granule(s): %s (%d)\n", channels, mode_gr, rc ? "FAILED" : "ok", rc);
            bad |= rc;
            rc = check_random(channels, mode_gr, 300, 1);
            printf("any index byte, %d channel(s), %d granule(s): %s (%d)\n", channels, mode_gr, rc ? "FAILED" : "ok", rc);
            bad |= rc;
        }
    rc = check_bins();
    printf("every bin: %s (%d)\n", rc ? "FAILED" : "ok", rc);
    bad |= rc;
    return bad ? 1 : 0;
}
