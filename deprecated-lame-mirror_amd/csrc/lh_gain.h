/*
 * lh_gain.h -- the radio gain of a batch, measured on the device (lh_gain.hip): the records of a launch, which the
 * host fills (lh_batch.cpp) and the kernel reads, and the leaf macros that name every rounding of the filters'
 * arithmetic.  lh_replaygain.c:44-97 (piece_energy) is the specification of that arithmetic; the kernel restates it
 * with these macros, and lh_gain_eval_host (lh_replaygain.c) is its twin on the host, made of piece_energy itself.
 *
 * What the analysis hears is decided by a plan the host makes from a stream's length alone (lh_gain_plan): the
 * blocks lame_encode_buffer would have handed to the analysis, flush included.  The kernel's result is the list of
 * per-window sums (lsum, rsum); bins, the 95 % level and the tenths of a dB are the host's (lh_rg_bin, lh_rg_tenths).
 */
#ifndef LH_GAIN_H
#define LH_GAIN_H

#include "lh_rs_sample.h"       /* LhRsMatrix, lh_rs_mix: the PCM matrix in front of the analysis */

/* The roundings of piece_energy, as C's types make them: a tap's product is a float product, rounded to float (it may be
 * subnormal); where the source adds two or three products in one expression (p[-2] * k + p[-1] * k) that sum is a float sum
 * as well, and only its result is widened -- exactly -- to double; the sums of those doubles are double; a filter's output
 * is the double difference rounded to float; the square of a piece's head sample is a double product, the squares in the
 * groups of four are float products, widened. */
#if defined(LH_RS_DEVICE) && defined(__HIP_DEVICE_COMPILE__)
#define LH_GN_FMUL(a, b) __fmul_rn((a), (b))
#define LH_GN_FADD(a, b) __fadd_rn((a), (b))
#define LH_GN_DADD(a, b) __dadd_rn((a), (b))
#define LH_GN_DSUB(a, b) __dsub_rn((a), (b))
#define LH_GN_DMUL(a, b) __dmul_rn((a), (b))
#define LH_GN_NARROW(a)  __double2float_rn(a)
#else
#define LH_GN_FMUL(a, b) ((a) * (b))
#define LH_GN_FADD(a, b) ((a) + (b))
#define LH_GN_DADD(a, b) ((a) + (b))
#define LH_GN_DSUB(a, b) ((a) - (b))
#define LH_GN_DMUL(a, b) ((a) * (b))
#define LH_GN_NARROW(a)  ((float) (a))
#endif
/* one product widened; two products added in float, widened */
#define LH_GN_TAP(x, k)  ((double) LH_GN_FMUL((x), (k)))
#define LH_GN_TAP2(x0, k0, x1, k1) ((double) LH_GN_FADD(LH_GN_FMUL((x0), (k0)), LH_GN_FMUL((x1), (k1))))

#define LH_GN_ORDER 10          /* samples of history the first filter needs */
#define LH_GN_RUN 64            /* samples a wave takes through the filters at a time: one per lane */
#define LH_GN_WAVES 4           /* streams (waves) per workgroup */
/* Launches of fewer streams than this run the first filter's feedback with its taps across the lanes of a row, larger ones in
 * lanes 0 and 1.  Measured on one MI355X (44.1 kHz stereo, ns per sample and stream): across the lanes 129 at 64, 256, 512 and
 * 1024 streams; in lanes 0 and 1 175 at 64 streams, 143 at 256, 120 at 512, 114 at 1024. */
#define LH_GN_TAPS_BELOW 384
#define LH_GN_MAX_TOTAL 0x7fffff00L     /* a stream's positions are ints on the device */

/* A stream of a launch.  Its blocks are `ntrunk' leading ones -- trunk[0 .. ntrunk), the made counts of the conversion
 * plan's shared trunk, or, where the launch has no trunk, `fs' samples each -- followed by tails[tail_at .. tail_at +
 * ntail); their lengths add up to `total'. */
typedef struct LhGainStream {
    long long n;                /* samples in the pool's rows: nothing at or beyond is ever read (zeros are generated) */
    long long win_at;           /* the stream's first window in the launch's output: total / window pairs from there (a
                                 * round: the windows that end in it) */
    int     total;              /* samples the analysis hears: n and the flush's zeros (a round: the round's blocks alone) */
    int     stream;             /* row pair of the pool */
    int     ntrunk;
    int     tail_at;
    int     ntail;
    int     pad_;
} LhGainStream;

/* What a stream of an incremental batch carries from round to round (lh_gain_resume_kernel; one record per stream, zeroed
 * = before the stream's first sample): per channel the last ten inputs behind the PCM matrix, the last ten outputs of the
 * first filter and the last two of the second, oldest first -- LhReplayGain's hist_in / hist_mid / hist_out[8..9] --, the
 * open window's sums, the samples heard and the windows finished so far.  A round ends at a block's end, so no piece's sum
 * is open between rounds.  Mono: channel 0 alone is kept, rsum = lsum. */
typedef struct LhGainCarry {
    float   x[2][LH_GN_ORDER], mid[2][LH_GN_ORDER], out[2][2];
    double  lsum, rsum;
    long long heard;
    long long windows;
} LhGainCarry;

/* what a launch needs besides its streams */
typedef struct LhGainParams {
    LhRsMatrix m;               /* s16 pool: the PCM matrix (a float pool is behind it already) */
    float   ky[21], kb[5];      /* the rate's rows of lh_rg_yule / lh_rg_butter */
    long long cap;              /* row length of the pool */
    int     window;             /* samples per 50 ms window at the output rate, rounded up */
    int     fs;                 /* length of a leading block where there is no trunk */
    int     channels;           /* 1: plane 0 stands for both sums */
    int     one_plane;          /* s16 pool, mono without a downmix: the second plane is never read */
    int     taps;               /* the first filter's feedback with its taps across the lanes of a row (else in lanes 0 and 1) */
} LhGainParams;

#endif
