/*
 * rs_plan_check.c -- TEST TOOL: the conversion plan that follows the calls of an incremental batch (csrc/lh_resample.c:
 * lh_rs_plan_call, lh_rs_plan_flush, lh_rs_block_tiles) run as a program of its own, built with AddressSanitizer and UBSan
 * (tests/rs_plan_check/Makefile), over the rate pairs and call patterns of tests/test_append_resample_plan.py.  It checks
 * what needs no reference: asking with room for no block, for one and for all gives the same count and the same blocks
 * and writes nothing beyond the room given; the blocks of a call follow each other on the input and on the output and
 * use the call up; the tiles of a block partition its outputs in order, each within LH_RS_SPAN_MAX, written only as far
 * as there is room; the flush from a copy of the cursor ends where the flush from the cursor does.  Prints one line per
 * pattern; exit status 0 = ok.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"

#define FS 1152
#define MFN 1904

static unsigned long long lcg = 0x4C414D45ULL;

static unsigned
draw(unsigned n)
{
    lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
    return (unsigned) ((lcg >> 33) % n);
}

static int
span_of(const LhResampler * r, const LhRsTile * t)
{
    LhRsSpot const a = lh_rs_locate(r->ratio, r->taps, r->phases, t->start, t->k0);
    LhRsSpot const z = lh_rs_locate(r->ratio, r->taps, r->phases, t->start, t->k0 + t->count - 1);
    return z.first + r->taps + 1 - a.first;
}

/* the tiles of the blocks: 0, or the number of the check that failed */
static int
check_tiles(const LhResampler * r, const LhRsBlock * blk, int nblk, long *ntiles, int *most)
{
    int     i, j;
    for (i = 0; i < nblk; i++) {
        int const n = lh_rs_block_tiles(r, &blk[i], 7, NULL, 0);
        LhRsTile one[2], *all;
        int     k = 0;
        if ((blk[i].made > 0) != (n > 0))
            return 10;
        memset(one, 0x5a, sizeof(one));
        if (lh_rs_block_tiles(r, &blk[i], 7, one, 1) != n || one[1].count != 0x5a5a5a5a)
            return 11;
        all = (LhRsTile *) malloc((size_t) (n > 0 ? n : 1) * sizeof(LhRsTile));
        if (!all)
            return 12;
        if (lh_rs_block_tiles(r, &blk[i], 7, all, n) != n)
            return 13;
        for (j = 0; j < n; j++) {
            if (all[j].k0 != k || all[j].count < 1 || all[j].out_at != blk[i].out_at + k || all[j].in_at != blk[i].in_at
                || all[j].start != blk[i].start || all[j].stream != 7)
                return 14;
            if (span_of(r, &all[j]) > LH_RS_SPAN_MAX)
                return 15;
            /* as large as fits: one more output would not have */
            if (j + 1 < n) {
                LhRsTile more = all[j];
                more.count++;
                if (span_of(r, &more) <= LH_RS_SPAN_MAX)
                    return 16;
            }
            k += all[j].count;
        }
        if (k != blk[i].made)
            return 17;
        if (n > 0 && memcmp(&one[0], &all[0], sizeof(LhRsTile)) != 0)
            return 18;
        *ntiles += n;
        if (n > *most)
            *most = n;
        free(all);
    }
    return 0;
}

static int
check_pattern(int rate_in, int rate_out, int ncalls)
{
    static const int sizes[] = { 0, 1, 3, 33, 575, 1151, 1152, 1153, 4000, 9000, 50000 };
    LhResampler *r = (LhResampler *) malloc(sizeof(LhResampler));
    LhRsCursor c, probe, end;
    long    nblocks = 0, ntiles = 0;
    int     call, most = 0, padding = -1, padding2 = -1, rc, n, n2, i;
    if (!r)
        return 1;
    lh_rs_init(r, rate_in, rate_out);
    lh_rs_cursor_init(&c);
    for (call = 0; call <= ncalls; call++) {
        int const flush = (call == ncalls);
        int const m = flush ? 0 : sizes[draw(sizeof(sizes) / sizeof(sizes[0]))];
        LhRsCursor const before = c;
        LhRsBlock few[2], *blk;
        probe = c;
        n = flush ? lh_rs_plan_flush(r, FS, MFN, &probe, NULL, 0, &padding) : lh_rs_plan_call(r, FS, MFN, &probe, m, NULL, 0);
        if (n < 0 || (!flush && (m > 0) != (n > 0)))
            return 2;
        memset(few, 0x5a, sizeof(few));
        end = c;
        n2 = flush ? lh_rs_plan_flush(r, FS, MFN, &end, few, 1, &padding2) : lh_rs_plan_call(r, FS, MFN, &end, m, few, 1);
        if (n2 != n || few[1].made != 0x5a5a5a5a || memcmp(&end, &probe, sizeof(end)) != 0 || padding2 != padding)
            return 3;
        blk = (LhRsBlock *) malloc((size_t) (n > 0 ? n : 1) * sizeof(LhRsBlock));
        if (!blk)
            return 4;
        n2 = flush ? lh_rs_plan_flush(r, FS, MFN, &c, blk, n, &padding2) : lh_rs_plan_call(r, FS, MFN, &c, m, blk, n);
        if (n2 != n || memcmp(&c, &probe, sizeof(c)) != 0 || (n > 0 && memcmp(&blk[0], &few[0], sizeof(LhRsBlock)) != 0))
            return 5;
        /* the blocks follow each other; those of a call use the call up */
        {
            long long in_at = before.in_at, out_at = before.fed;
            for (i = 0; i < n; i++) {
                if (blk[i].out_at != out_at || blk[i].in_at < in_at || blk[i].made < 0 || blk[i].made > FS || blk[i].len < 1)
                    return 6;
                if (!flush && blk[i].len != (int) (before.in_at + m - blk[i].in_at))
                    return 7;
                in_at = blk[i].in_at;
                out_at += blk[i].made;
            }
            if (out_at != c.fed || (!flush && c.in_at != before.in_at + m) || c.nblk != before.nblk + n)
                return 8;
        }
        if (flush && (padding < 576 || padding >= 576 + FS || c.frames < 1))
            return 9;
        if ((rc = check_tiles(r, blk, n, &ntiles, &most)) != 0)
            return rc;
        nblocks += n;
        free(blk);
    }
    printf("%d -> %d Hz, %d calls: %lld input samples, %lld converted, %d frames, padding %d, %ld blocks, %ld tiles (at most %d a block)\n",
           rate_in, rate_out, ncalls, c.in_at, c.fed, c.frames, padding, nblocks, ntiles, most);
    free(r);
    return 0;
}

int
main(void)
{
    static const int pairs[][2] = { {48000, 44100}, {44100, 48000}, {96000, 32000}, {44100, 32000}, {32000, 44100}, {8000, 32000} };
    size_t  p;
    int     round;
    for (p = 0; p < sizeof(pairs) / sizeof(pairs[0]); p++)
        for (round = 0; round < 3; round++) {
            int const rc = check_pattern(pairs[p][0], pairs[p][1], round == 0 ? 0 : 20);
            if (rc) {
                printf("FAILED (check %d): %d -> %d Hz, pattern %d\n", rc, pairs[p][0], pairs[p][1], round);
                return 1;
            }
        }
    printf("ok\n");
    return 0;
}
