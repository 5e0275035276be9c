/*
 * lh_gain_stream.h -- the text of the gain kernels (lh_gain.hip includes it twice): with GN_RESUME 0 lh_gain_kernel, a
 * whole stream from silence; with GN_RESUME 1 lh_gain_resume_kernel, a round of a stream from and to its LhGainCarry.
 * One text, so that the two cannot drift apart, and two compilations of it, so that the whole-stream kernel is exactly
 * what the compiler made of it before there was a second one.  The head comment of lh_gain.hip describes both.
 */
#if GN_RESUME
#define GN_REAL real
/* (windows end at multiples of W of the samples heard: w0 may lie before the round's start) */
#define GN_W0(pos) (((base + (pos)) / W) * W - base)
#else
#define GN_REAL sd.n
#define GN_W0(pos) (((pos) / W) * W)
#endif

/* grid: x = LH_GN_WAVES entries of `streams' (GN_RESUME: the streams with work in the round; carry: one record per stream of
 * the batch, indexed like the pool) */
template < typename T, int TAPS >
#ifndef LH_EMU
__global__ void __launch_bounds__(LH_GN_NT)
#else
void
#endif
#if GN_RESUME
lh_gain_resume_kernel(LhGainParams p, const LhGainStream * streams, int nstreams, const int *tails, const T * pool, double *pairs,
                      LhGainCarry * carry)
#else
lh_gain_kernel(LhGainParams p, const LhGainStream * streams, int nstreams, const int *trunk, const int *tails, const T * pool,
               double *pairs)
#endif
{
    __shared__ LhGainLds lds[LH_GN_WAVES];
    int const lane = lh_lane(), wave = lh_wave_id();
    int const si = (int) blockIdx.x * LH_GN_WAVES + wave;
    if (si >= nstreams)
        return;                 /* (the whole wave: nothing below waits for another wave) */
    LhGainLds & L = lds[wave];
    LhGainStream const sd = streams[si];
    int const nch = p.channels == 1 ? 1 : 2, W = p.window;
    int const nblk = sd.ntrunk + sd.ntail;
#if GN_RESUME
    /* the round's blocks are all listed (no trunk); positions below are counted from the round's start, `base' samples into
     * the stream, and the pool's rows are real up to `real' of them */
    const int *const trunk = (const int *) 0;
    LhGainCarry *const cy = carry + sd.stream;
    int const base = (int) cy->heard;
    long long const real = sd.n - base;
    const T *row_l = pool + (size_t) sd.stream * 2 * (size_t) p.cap + base, *row_r = row_l + p.cap;
#else
    const T *row_l = pool + (size_t) sd.stream * 2 * (size_t) p.cap, *row_r = row_l + p.cap;
#endif
    double *out = pairs + 2 * sd.win_at;
    /* what lanes 0 and 1 carry from run to run: the filters' histories and the sums; every lane: the block cursor */
    float   q[LH_GN_ORDER], o1 = 0.0f, o2 = 0.0f;
    double  sum = 0.0, wsum = 0.0;
    int     wins = 0;
    int     blk = 0, blk_at = 0, blk_len = nblk > 0 ? gain_block_len(sd, p.fs, trunk, tails, 0) : 0;
    /* TAPS: lane r < 10 of a row of 16 holds the first filter's output 10 - r samples back and its feedback tap; rows 0 and 1
     * are the channels (rows 2 and 3 shadow them and store nothing) */
    int const tap = lane & 15, tap_ch = (lane >> 4) & 1;
    bool const tap_writer = tap == 8 && (lane >> 4) < nch;
    float   kt = 0.0f, h = 0.0f;
#pragma unroll
    for (int j = 0; j < LH_GN_ORDER; ++j) {
        q[j] = 0.0f;
        if (tap == j)
            kt = p.ky[11 + j];
    }
#if GN_RESUME
    /* the carry's samples at the ring's slots for positions -10 .. -1, zeros elsewhere */
    for (int c = 0; c < 2; ++c)
        for (int k = lane; k < LH_GN_RING; k += 64) {
            int const j = k - (LH_GN_RING - LH_GN_ORDER);
            L.x[c][k] = j >= 0 ? cy->x[c][j] : 0.0f;
            L.mid[c][k] = j >= 0 ? cy->mid[c][j] : 0.0f;
            L.out[c][k] = j >= LH_GN_ORDER - 2 ? cy->out[c][j - (LH_GN_ORDER - 2)] : 0.0f;
        }
    LH_WAVE_SYNC();
    {
        /* the histories both mappings of C and E start from, and the open window's sums (lane 0 left, lane 1 right) */
        const float *m = L.mid[TAPS ? tap_ch : (lane & 1)], *o = L.out[lane & 1];
#pragma unroll
        for (int j = 0; j < LH_GN_ORDER; ++j)
            q[j] = GN_AT(m, 0, 1 + j);
        h = tap < LH_GN_ORDER ? GN_AT(m, 0, LH_GN_ORDER - tap) : 0.0f;
        o1 = GN_AT(o, 0, 1);
        o2 = GN_AT(o, 0, 2);
        wsum = (lane & 1) ? cy->rsum : cy->lsum;
    }
#else
    for (int c = 0; c < 2; ++c)
        for (int k = lane; k < LH_GN_RING; k += 64)
            L.x[c][k] = L.mid[c][k] = L.out[c][k] = 0.0f;
    LH_WAVE_SYNC();
#endif
    for (int at = 0; at < sd.total; at += LH_GN_RUN) {
        int const pos = at + lane, slot = pos & (LH_GN_RING - 1), half = at & LH_GN_RUN;
        /* A */
        {
            float   xl = 0.0f, xr = 0.0f;
            if (pos < GN_REAL) {
                if (sizeof(T) == 2) {
                    float const sl = (float) row_l[pos], sr = p.one_plane ? sl : (float) row_r[pos];
                    xl = lh_rs_mix(sl, sr, p.m.m00, p.m.m01);
                    if (nch == 2)
                        xr = lh_rs_mix(sl, sr, p.m.m10, p.m.m11);
                }
                else {
                    xl = (float) row_l[pos];
                    if (nch == 2)
                        xr = (float) row_r[pos];
                }
            }
            L.x[0][slot] = xl;
            L.x[1][slot] = xr;
        }
        LH_WAVE_SYNC();
        /* B */
        for (int c = 0; c < nch; ++c)
            L.d[c][lane] = gain_yule_forward(L.x[c], pos, p.ky);
        LH_WAVE_SYNC();
        /* C */
        if (TAPS) {
            /* one instruction stream for both channels: the ten products at once, the pairs (float sums) on the even lanes,
             * then the ordered double sum walks up the row two lanes at a time -- x1 in lane 0, + x5 in lane 2, + x9, + xD,
             * + xH in lane 8, which forms the output; the history moves down a lane and takes the output in at lane 9 */
            const double *s1 = L.d[tap_ch];
            float  *mid = L.mid[tap_ch] + half;
#pragma unroll 8
            for (int i = 0; i < LH_GN_RUN; ++i) {
                float const pr = LH_GN_FMUL(h, kt);
                double const x = (double) LH_GN_FADD(pr, lh_row_shl_f32 < 1 > (pr));
                double  acc = x;
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                acc = LH_GN_DADD(lh_row_shr_f64 < 2 > (acc), x);
                float const v = LH_GN_NARROW(LH_GN_DSUB(s1[i], acc));
                if (tap_writer)
                    mid[i] = v;
                float const older = lh_row_shl_f32 < 1 > (h), newest = lh_row_shr_f32 < 1 > (v);
                h = tap == 9 ? newest : older;
            }
        }
        else if (lane < nch) {
            const double *s1 = L.d[lane];
            float  *mid = L.mid[lane] + half;
            for (int i0 = 0; i0 < LH_GN_RUN; i0 += 16) {
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    float const v = LH_GN_NARROW(LH_GN_DSUB(s1[i0 + u], gain_yule_feedback(q, p.ky)));
#pragma unroll
                    for (int j = LH_GN_ORDER - 1; j > 0; --j)
                        q[j] = q[j - 1];
                    q[0] = v;
                    mid[i0 + u] = v;
                }
            }
        }
        LH_WAVE_SYNC();
        /* D */
        for (int c = 0; c < nch; ++c) {
            const float *m = L.mid[c];
            /* (three products in one float expression) */
            L.d[c][lane] = (double) LH_GN_FADD(LH_GN_FADD(LH_GN_FMUL(GN_AT(m, pos, 2), p.kb[0]), LH_GN_FMUL(GN_AT(m, pos, 1), p.kb[2])),
                                               LH_GN_FMUL(GN_AT(m, pos, 0), p.kb[4]));
        }
        LH_WAVE_SYNC();
        /* E */
        if (lane < nch) {
            const double *s1 = L.d[lane];
            float  *o = L.out[lane] + half;
#pragma unroll 16
            for (int i = 0; i < LH_GN_RUN; ++i) {
                double const s2 = LH_GN_TAP2(o2, p.kb[1], o1, p.kb[3]);
                float const v = LH_GN_NARROW(LH_GN_DSUB(s1[i], s2));
                o2 = o1;
                o1 = v;
                o[i] = v;
            }
        }
        LH_WAVE_SYNC();
        /* F */
        bool const valid = pos < sd.total;
        int     j = blk, b0 = blk_at, bn = blk_len;
        while (valid && pos >= b0 + bn && j + 1 < nblk) {
            b0 += bn;
            ++j;
            bn = gain_block_len(sd, p.fs, trunk, tails, j);
        }
        int const w0 = GN_W0(pos), in_blk = pos - b0;
        int     first = b0 + (in_blk >= LH_GN_ORDER ? LH_GN_ORDER : 0), end = b0 + bn;
        if (w0 > first)
            first = w0;
        if (in_blk < LH_GN_ORDER && b0 + LH_GN_ORDER < end)
            end = b0 + LH_GN_ORDER;
        if (w0 + W < end)
            end = w0 + W;
        int const k = pos - first, head = (end - first) & 3;
        bool const single = valid && k < head, four = valid && k >= head && ((k - head) & 3) == 3;
        for (int c = 0; c < nch; ++c) {
            const float *o = L.out[c];
            double  t = 0.0;
            if (single) {
                double const v = (double) GN_AT(o, pos, 0);
                t = LH_GN_DMUL(v, v);
            }
            else if (four) {
                float const fa = GN_AT(o, pos, 3), fb = GN_AT(o, pos, 2), fc = GN_AT(o, pos, 1), fd = GN_AT(o, pos, 0);
                t = LH_GN_DADD(LH_GN_DADD(LH_GN_DADD(LH_GN_TAP(fa, fa), LH_GN_TAP(fb, fb)), LH_GN_TAP(fc, fc)), LH_GN_TAP(fd, fd));
            }
            L.d[c][lane] = t;
        }
        uint64_t const m_term = lh_ballot(single || four), m_last = lh_ballot(valid && pos == end - 1);
        uint64_t const m_win = lh_ballot(valid && pos == w0 + W - 1);
        LH_WAVE_SYNC();
        /* G */
        if (lane < nch) {
            uint64_t m = m_term | m_last;
            while (m) {
                int const i = lh_ffs64(m);
                m &= m - 1;
                if ((m_term >> i) & 1)
                    sum = LH_GN_DADD(sum, L.d[lane][i]);
                if ((m_last >> i) & 1) {
                    wsum = LH_GN_DADD(wsum, sum);
                    sum = 0.0;
                    if ((m_win >> i) & 1) {
                        out[2 * (long long) wins + lane] = wsum;
                        if (nch == 1)
                            out[2 * (long long) wins + 1] = wsum;
                        wsum = 0.0;
                        ++wins;
                    }
                }
            }
        }
        blk = (int) lh_bcast_u32((uint32_t) j, 63);
        blk_at = (int) lh_bcast_u32((uint32_t) b0, 63);
        blk_len = (int) lh_bcast_u32((uint32_t) bn, 63);
        LH_WAVE_SYNC();
    }
#if GN_RESUME
    /* the carry, from the ring at the round's end (a round shorter than ten samples keeps part of the old one there) */
    for (int c = 0; c < nch; ++c) {
        if (lane < LH_GN_ORDER) {
            cy->x[c][lane] = GN_AT(L.x[c], sd.total, LH_GN_ORDER - lane);
            cy->mid[c][lane] = GN_AT(L.mid[c], sd.total, LH_GN_ORDER - lane);
        }
        if (lane < 2)
            cy->out[c][lane] = GN_AT(L.out[c], sd.total, 2 - lane);
    }
    if (lane < nch) {
        if (lane == 0)
            cy->lsum = wsum;
        if (lane == 1 || nch == 1)
            cy->rsum = wsum;
    }
    if (lane == 0) {
        cy->heard = (long long) base + sd.total;
        cy->windows += wins;
    }
#endif
}

#undef GN_REAL
#undef GN_W0
