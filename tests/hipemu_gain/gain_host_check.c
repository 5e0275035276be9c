/*
 * gain_host_check.c -- TEST TOOL: the host side of a batch's ReplayGain analysis (lh_gain_plan, lh_gain_eval_host) run as
 * a program of its own over a list of stream lengths, with and without rate conversion, built with AddressSanitizer and
 * UBSan (tests/hipemu_gain/Makefile).  It checks what needs no reference: a plan's blocks add up to its total, asking
 * again with room for every block gives the same blocks, the twin returns total / window windows, writes no pair beyond
 * its cap, and its gain is the one lh_gain_from_windows makes of the pairs.  Prints one line per case; exit status 0 = ok.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lh_host.h"

static int
check(int rate_in, int rate_out, int channels, int fs, long n)
{
    int const mfn = LH_BLKSIZE + fs - LH_FFTOFFSET;
    long const window = (rate_out + 19L) / 20L;
    LhResampler *rs = NULL;
    int     few[2] = { -7, -7 }, *blocks, nb, nb2, i, tenths = -1, tenths2 = -1;
    long    total = -1, total2 = -1, sum = 0, nwin, nwin2, k;
    float  *l, *r;
    double *pairs;
    if (rate_in != rate_out) {
        rs = (LhResampler *) malloc(sizeof(LhResampler));
        if (!rs)
            return 1;
        lh_rs_init(rs, rate_in, rate_out);
    }
    nb = lh_gain_plan(rs, fs, mfn, n, few, 1, &total);  /* room for one block: the rest is only counted */
    if (nb < 0 || few[1] != -7)
        return 2;
    blocks = (int *) malloc((size_t) (nb + 1) * sizeof(int));
    blocks[nb] = -7;
    nb2 = lh_gain_plan(rs, fs, mfn, n, blocks, nb, &total2);
    if (nb2 != nb || total2 != total || blocks[nb] != -7 || (nb > 0 && blocks[0] != few[0]))
        return 3;
    for (i = 0; i < nb; i++) {
        if (blocks[i] < 0 || blocks[i] > 1152)
            return 4;
        sum += blocks[i];
    }
    if (sum != total || (!rs && total < n))
        return 5;
    /* the samples: as many as the analysis may read (all of them when the plan is a conversion's: its input is the
     * converted signal), exactly allocated so that a read beyond them is seen */
    k = rs ? total : n;
    l = (float *) malloc((size_t) (k > 0 ? k : 1) * sizeof(float));
    r = (float *) malloc((size_t) (k > 0 ? k : 1) * sizeof(float));
    for (i = 0; i < k; i++) {
        l[i] = (float) (9000.0 * sin(0.05 * i) + 3000.0 * sin(0.61 * i + 1.0));
        r[i] = (float) (7000.0 * sin(0.031 * i + 0.5));
    }
    pairs = (double *) malloc((size_t) (2 * (total / window) + 4) * sizeof(double));
    nwin = lh_gain_eval_host(rate_out, channels, blocks, nb, l, r, k, pairs, total / window, &tenths);
    if (nwin != total / window)
        return 6;
    if (tenths != lh_gain_from_windows(pairs, nwin, window))
        return 7;
    for (i = 0; i < nwin; i++)
        if (!(pairs[2 * i] >= 0.0) || (channels == 1 && pairs[2 * i] != pairs[2 * i + 1]))
            return 8;
    /* a cap of one: the count is the same, the second pair stays untouched */
    pairs[2] = pairs[3] = -1.0;
    nwin2 = lh_gain_eval_host(rate_out, channels, blocks, nb, l, r, k, pairs, 1, &tenths2);
    if (nwin2 != nwin || tenths2 != tenths || pairs[2] != -1.0 || pairs[3] != -1.0)
        return 9;
    printf("%d -> %d Hz, %d ch, fs %d, %ld samples: %d blocks, %ld heard, %ld windows, %d tenths of a dB\n", rate_in, rate_out,
           channels, fs, n, nb, total, nwin, tenths);
    free(pairs);
    free(l);
    free(r);
    free(blocks);
    free(rs);
    return 0;
}

int
main(void)
{
    static const int settings[][4] = { {44100, 44100, 2, 1152}, {48000, 48000, 2, 1152}, {32000, 32000, 1, 1152},
    {22050, 22050, 2, 576}, {48000, 44100, 2, 1152}, {44100, 32000, 2, 1152}
    };
    size_t  s;
    int     i;
    for (s = 0; s < sizeof(settings) / sizeof(settings[0]); s++) {
        int const fs = settings[s][3];
        long const w = (settings[s][1] + 19L) / 20L;
        long const lengths[] = { 0, 1, 9, 10, 11, fs - 1, fs, fs + 1, w - 1, w, w + 1, w + 10, 2 * w, 3 * fs, settings[s][0] * 7L / 10 };
        for (i = 0; i < (int) (sizeof(lengths) / sizeof(lengths[0])); i++) {
            int const rc = check(settings[s][0], settings[s][1], settings[s][2], fs, lengths[i]);
            if (rc) {
                printf("FAILED (check %d): %d -> %d Hz, %ld samples\n", rc, settings[s][0], settings[s][1], lengths[i]);
                return 1;
            }
        }
    }
    printf("ok\n");
    return 0;
}
