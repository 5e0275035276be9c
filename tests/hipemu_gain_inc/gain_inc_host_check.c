/*
 * gain_inc_host_check.c -- TEST TOOL: the host side of an incremental batch's ReplayGain analysis run as a program of its
 * own, built with AddressSanitizer and UBSan (tests/hipemu_gain_inc/Makefile): the plan that follows the calls
 * (lh_gain_plan_call, lh_gain_plan_flush; for a converting setting the made counts of lh_rs_plan_call / lh_rs_plan_flush)
 * over lists of calls, and the host twin (lh_gain_eval_host) over the blocks of all calls and the flush.  It checks what
 * needs no reference: asking with no room only counts and moves the cursor alike, no block beyond the room is written, a
 * call's blocks add up to the call, the cursor counts what the blocks add up to, a stream fed a frame per call is
 * lh_gain_plan's, and the twin returns heard / window windows.  Prints one line per case; exit status 0 = ok.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"

#define MAXBLK 4096

static int
check(int rate_in, int rate_out, int channels, int fs, const int *calls, int ncalls)
{
    int const mfn = LH_BLKSIZE + fs - LH_FFTOFFSET;
    long const window = (rate_out + 19L) / 20L;
    int    *blocks = (int *) malloc((MAXBLK + 1) * sizeof(int));
    LhRsBlock *rb = (LhRsBlock *) malloc(MAXBLK * sizeof(LhRsBlock));
    LhResampler *rs = NULL;
    LhGainCursor c, probe;
    LhRsCursor rc;
    long    heard = 0, fed_in = 0, nwin, i;
    int     nb = 0, k, j, tenths = -1, padding = 0;
    float  *l, *r;
    double *pairs;
    if (!blocks || !rb)
        return 1;
    lh_gain_cursor_init(&c);
    lh_rs_cursor_init(&rc);
    if (rate_in != rate_out) {
        rs = (LhResampler *) malloc(sizeof(LhResampler));
        if (!rs)
            return 1;
        lh_rs_init(rs, rate_in, rate_out);
    }
    for (i = 0; i <= ncalls; i++) {     /* (the last turn is the flush) */
        int const m = i < ncalls ? calls[i] : 0;
        long    sum = 0;
        if (rs) {
            k = i < ncalls ? lh_rs_plan_call(rs, fs, mfn, &rc, m, rb, MAXBLK - nb) : lh_rs_plan_flush(rs, fs, mfn, &rc, rb, MAXBLK - nb, &padding);
            if (k < 0 || nb + k > MAXBLK)
                return 2;
            for (j = 0; j < k; j++)
                if (rb[j].made > 0)
                    blocks[nb++] = rb[j].made;
            heard = (long) rc.fed;
        }
        else {
            probe = c;
            blocks[nb] = -7;
            k = i < ncalls ? lh_gain_plan_call(&probe, fs, mfn, m, NULL, 0) : lh_gain_plan_flush(&probe, fs, mfn, NULL, 0);
            if (k < 0 || nb + k > MAXBLK || blocks[nb] != -7)
                return 3;
            blocks[nb + k] = -7;
            j = i < ncalls ? lh_gain_plan_call(&c, fs, mfn, m, blocks + nb, k) : lh_gain_plan_flush(&c, fs, mfn, blocks + nb, k);
            if (j != k || blocks[nb + k] != -7 || memcmp(&c, &probe, sizeof(c)) != 0)
                return 4;
            for (j = 0; j < k; j++) {
                if (blocks[nb + j] < 1 || blocks[nb + j] > 1152)
                    return 5;
                sum += blocks[nb + j];
            }
            if (i < ncalls && (sum != m || k != (m + fs - 1) / fs))
                return 6;
            nb += k;
            heard += sum;
            if (c.heard != heard)
                return 7;
        }
        fed_in += m;
    }
    /* the samples the analysis may read: what was fed (the converted signal, flush included, where the setting converts),
     * exactly allocated so that a read beyond them is seen */
    i = rs ? heard : fed_in;
    l = (float *) malloc((size_t) (i > 0 ? i : 1) * sizeof(float));
    r = (float *) malloc((size_t) (i > 0 ? i : 1) * sizeof(float));
    pairs = (double *) malloc((size_t) (2 * (heard / window) + 2) * sizeof(double));
    if (!l || !r || !pairs)
        return 1;
    for (j = 0; j < i; j++) {
        l[j] = (float) (9000.0 * sin(0.05 * j) + 3000.0 * sin(0.61 * j + 1.0));
        r[j] = (float) (7000.0 * sin(0.031 * j + 0.5));
    }
    nwin = lh_gain_eval_host(rate_out, channels, blocks, nb, l, r, i, pairs, heard / window, &tenths);
    if (nwin != heard / window || tenths != lh_gain_from_windows(pairs, nwin, window))
        return 8;
    printf("%d -> %d Hz, %d ch, fs %d, %d calls of %ld samples: %d blocks, %ld heard, %ld windows, %d tenths of a dB\n", rate_in,
           rate_out, channels, fs, ncalls, fed_in, nb, heard, nwin, tenths);
    free(pairs);
    free(l);
    free(r);
    free(rs);
    free(rb);
    free(blocks);
    return 0;
}

/* a stream fed a frame's worth per call: the blocks of lh_gain_plan */
static int
check_whole(int fs, long n)
{
    int const mfn = LH_BLKSIZE + fs - LH_FFTOFFSET;
    int    *a = (int *) malloc(MAXBLK * sizeof(int)), *b = (int *) malloc(MAXBLK * sizeof(int));
    LhGainCursor c;
    long    total = -1, at;
    int     na, nb = 0, k;
    if (!a || !b)
        return 1;
    na = lh_gain_plan(NULL, fs, mfn, n, a, MAXBLK, &total);
    lh_gain_cursor_init(&c);
    for (at = 0; at < n; at += fs) {
        if ((k = lh_gain_plan_call(&c, fs, mfn, (int) (n - at > fs ? fs : n - at), b + nb, MAXBLK - nb)) < 0)
            return 9;
        nb += k;
    }
    if ((k = lh_gain_plan_flush(&c, fs, mfn, b + nb, MAXBLK - nb)) < 0)
        return 9;
    nb += k;
    k = (na != nb || total != (long) c.heard || memcmp(a, b, (size_t) na * sizeof(int)) != 0) ? 10 : 0;
    free(a);
    free(b);
    return k;
}

int
main(void)
{
    static const int settings[][4] = { {44100, 44100, 2, 1152}, {48000, 48000, 2, 1152}, {32000, 32000, 1, 1152},
    {22050, 22050, 2, 576}, {48000, 44100, 2, 1152}, {44100, 32000, 2, 1152}
    };
    size_t  s;
    int     i, o;
    for (s = 0; s < sizeof(settings) / sizeof(settings[0]); s++) {
        int const fs = settings[s][3], w = (settings[s][1] + 19) / 20;
        int const lengths[12] = { 0, 1, 9, 10, 11, fs - 1, fs, fs + 1, w - 1, w, w + 1, 3 * fs + 7 };
        int     calls[12], rc;
        for (o = 0; o < 3; o++) {       /* as listed, backwards, every fifth */
            for (i = 0; i < 12; i++)
                calls[i] = lengths[o == 0 ? i : o == 1 ? 11 - i : (5 * i + 3) % 12];
            if ((rc = check(settings[s][0], settings[s][1], settings[s][2], fs, calls, 12)) != 0) {
                printf("FAILED (check %d): %d -> %d Hz, order %d\n", rc, settings[s][0], settings[s][1], o);
                return 1;
            }
        }
        if ((rc = check(settings[s][0], settings[s][1], settings[s][2], fs, calls, 0)) != 0) {  /* the empty stream: flush only */
            printf("FAILED (check %d): %d -> %d Hz, empty stream\n", rc, settings[s][0], settings[s][1]);
            return 1;
        }
        for (i = 0; i < 12; i++)
            if ((rc = check_whole(fs, lengths[i])) != 0) {
                printf("FAILED (check %d): fs %d, %d samples whole\n", rc, fs, lengths[i]);
                return 1;
            }
    }
    printf("ok\n");
    return 0;
}
