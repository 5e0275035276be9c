/*
 * drain_host_check.c -- TEST TOOL: the host's half of a round's drain (csrc/lh_drain.h: lh_drain_bound, lh_drain_tiles)
 * over a list of cases, as a stand-alone program built with AddressSanitizer and UBSan (tests/hipemu_drain/Makefile).
 * The tile table is written into a buffer of exactly the size the counting call asked for, so that a table one entry too
 * long is a sanitizer report; every property the gather kernel's grid relies on is checked.  Prints "ok" and returns 0.
 */
#include <stdio.h>
#include <stdlib.h>
#include "lh_drain.h"

static int failures = 0;

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static void
check_tiles(const long long *bound, int n)
{
    long long padded = -1, padded2 = -1, want_padded = 0, covered;
    long long const count = lh_drain_tiles(bound, n, NULL, 0, &padded);
    LhDrainTile *t = (LhDrainTile *) malloc((size_t) (count > 0 ? count : 1) * sizeof(LhDrainTile));
    long long k = 0;
    int     s;
    CHECK(t != NULL);
    if (!t)
        return;
    CHECK(lh_drain_tiles(bound, n, t, count, &padded2) == count);
    CHECK(padded == padded2);
    for (s = 0; s < n; s++) {
        long long const b = bound[s] > 0 ? bound[s] : 0;
        covered = 0;
        /* the stream's tiles: in order, gapless, the last one reaching its bound */
        while (k < count && t[k].stream == s) {
            CHECK((long long) t[k].tile * LH_DR_TILE == covered);
            CHECK(covered < b);
            covered += LH_DR_TILE;
            k++;
        }
        CHECK(covered >= b && covered - b < LH_DR_TILE);
        want_padded += (b + LH_DR_PIECE - 1) / LH_DR_PIECE * LH_DR_PIECE;
    }
    CHECK(k == count);
    CHECK(padded == want_padded && padded % LH_DR_PIECE == 0);
    /* a shorter room: the count is the same, nothing behind the room is written (the buffer has `room' entries) */
    if (count > 1) {
        LhDrainTile *few = (LhDrainTile *) malloc((size_t) (count / 2) * sizeof(LhDrainTile));
        CHECK(few != NULL);
        if (few) {
            CHECK(lh_drain_tiles(bound, n, few, count / 2, NULL) == count);
            for (k = 0; k < count / 2; k++)
                CHECK(few[k].stream == t[k].stream && few[k].tile == t[k].tile);
            free(few);
        }
    }
    free(t);
}

int
main(void)
{
    /* the bound: frames x largest frame, inside the slice, less what is drained; never negative */
    CHECK(lh_drain_bound(0, 0, 418, 1000, 0) == 0);
    CHECK(lh_drain_bound(0, 2, 418, 100000, 0) == 836);
    CHECK(lh_drain_bound(0, 2, 418, 100000, 836) == 0);
    CHECK(lh_drain_bound(0, 2, 418, 100000, 900) == 0);
    CHECK(lh_drain_bound(0, 2, 418, 500, 100) == 400);
    CHECK(lh_drain_bound(0, -1, 418, 500, 0) == 0);
    CHECK(lh_drain_bound(0, 3, 0, 500, 0) == 0);
    CHECK(lh_drain_bound(0, 1000000, 1441, 1441000000ll, 5) == 1441000000ll - 5);
    /* behind a round that came home: from where the frames ended then */
    CHECK(lh_drain_bound(5000, 2, 418, 100000, 4700) == 1136);
    CHECK(lh_drain_bound(5000, 0, 418, 100000, 4700) == 300);
    CHECK(lh_drain_bound(5000, 2, 418, 5200, 4700) == 500);
    CHECK(lh_drain_bound(-3, 2, 418, 100000, 0) == 836);
    {
        long long const none[1] = { 0 };
        long long const one[1] = { 1 };
        long long const edge[6] = { LH_DR_TILE - 1, LH_DR_TILE, LH_DR_TILE + 1, 0, -5, 3 * LH_DR_TILE };
        long long many[300];
        int     i;
        for (i = 0; i < 300; i++)
            many[i] = (long long) ((i * 7919) % (5 * LH_DR_TILE)) - 100;
        check_tiles(none, 0);
        check_tiles(none, 1);
        check_tiles(one, 1);
        check_tiles(edge, 6);
        check_tiles(many, 300);
    }
    if (failures)
        return 1;
    printf("ok\n");
    return 0;
}
