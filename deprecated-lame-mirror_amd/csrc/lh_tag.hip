/*
 * lh_tag.hip -- the Xing/Info + LAME tag frames of a device-packed batch on the device (gfx950): behind the encode kernel,
 * lh_tag_kernel writes every stream's final tag frame into the room in front of its audio bytes, byte for byte what
 * lamehip_batch_get_bytes_tagged makes of the same bytes on the host (lh_vbrtag.c), so that the batch's fetch brings
 * complete file images home.  A workgroup of LH_TAG_NT lanes takes one stream:
 *   A  the music CRC-16 over the stream's audio bytes (reflected polynomial 0xA001, initial value 0: lh_tag_crc).  The
 *      CRC is linear over GF(2) and leading zero bytes leave it at 0, so the bytes -- less the few behind the last
 *      16-byte boundary of memory -- are thought of as padded in front to whole rows of LH_TAG_ROW bytes; in every row a
 *      lane takes the LH_TAG_PIECE bytes at its place, one 16-byte load the wave's lanes make side by side, and brings
 *      its own CRC from piece to piece over the rest of the row as if that were zeros (a 16 x 16 bit matrix, columns in
 *      scalar registers: LhTagParams.adv).  The lanes' CRCs then fold pairwise, acc = advance(lower, bytes of the upper)
 *      ^ upper, through six butterfly steps in a wave and across the waves in LDS, and lane 0 takes the bytes behind the
 *      last boundary one by one.  A piece that reaches out of the stream is loaded byte by byte, inside it only: nothing
 *      in front of the slice and nothing at or behind em_next_header is ever read.  The byte step (lh_tag_crc_byte) needs
 *      no table: 64 lanes indexing a 256-entry table in LDS by byte would collide on its banks, and the polynomial's
 *      three taps make a byte a dozen VALU instructions.
 *   B  the bookkeeping of lh_tag_add_frame over the launch's LhFrameOut records, in closed form: after n frames the
 *      sampling distance `want' is the smallest power of two with n / want < 400, the bag holds pos = n / want samples,
 *      and sample j is the sum of the first (j + 1) want bit rates -- a prefix sum, 256 frames per step.
 *   C  the frame: the host's template (lh_tag_template) into LDS, the seek table's 99 entries a lane each, the other
 *      fields and the two CRCs over the frame in lane 0 (lh_tag.h, the text lh_tag_frame runs on the host), and out.
 * A stream without frames gets zeros, as does one whose packer reported a status (which the getters report).
 * An incremental batch that packs on the device (lamehip_batch_set_incremental_tagging) has no round in which all of a
 * stream's bytes and records are there: lh_tag_resume_kernel runs behind every round's drain and moves a carry per stream
 * in HBM on (lh_tag.h: LhTagCarry) -- A over the bytes that became final with the round, joined to the carried CRC moved on
 * over as many zeros (LhTagPow: the advance by powers of two, through the set bits of the count); B over the round's
 * records, the carried bag thinned out first when the sampling distance grows --, and behind the flush makes C of the carry.
 * Built with -ffp-contract=off like every object of the library; lh_tag.h names the seek table's roundings.
 */
#include <stdint.h>
#include <math.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_TAG_FN static inline
#else
#include <hip/hip_runtime.h>
#define LH_TAG_DEVICE
#define LH_TAG_FN static __device__ __forceinline__
#endif
#include "lh_wave.h"
#include "lh_device.h"
#include "lh_tag.h"
#include "lh_drain.h"

#define LH_TAG_WAVES (LH_TAG_NT / 64)
#define LH_TAG_MAX_FRAME 2880   /* lh_tag_init allows no larger frame */

struct LhTagLds {
    unsigned char frame[LH_TAG_MAX_FRAME];
    int     bag[LH_TAG_BAG_SIZE];
    int     wave_sum[LH_TAG_WAVES];
    uint32_t wave_crc[LH_TAG_WAVES];
};

struct LhTagPiece {
    uint32_t w[4];
};

typedef uint32_t lh_tag_v4 __attribute__((vector_size(16)));

/* the piece `off' bytes from `bytes' (at a multiple of 16 in memory) of the bytes [0, hi) there: what lies outside counts as
 * zero and is not read */
LH_TAG_FN LhTagPiece
tag_piece(const unsigned char *bytes, long long off, long long hi)
{
    LhTagPiece v = { {0, 0, 0, 0} };
    if (off >= 0 && off + LH_TAG_PIECE <= hi) {
        lh_tag_v4 const t = *(const lh_tag_v4 *) __builtin_assume_aligned(bytes + off, LH_TAG_PIECE);
        v.w[0] = t[0];
        v.w[1] = t[1];
        v.w[2] = t[2];
        v.w[3] = t[3];
    }
    else if (off + LH_TAG_PIECE > 0 && off < hi) {
        for (int j = 0; j < LH_TAG_PIECE; j++)
            if (off + j >= 0 && off + j < hi)
                v.w[j >> 2] |= (uint32_t) bytes[off + j] << (8 * (j & 3));
    }
    return v;
}

/* A: the music CRC of the n bytes at `bytes'; all lanes of the workgroup call it, lane 0 gets the result */
LH_TAG_FN uint32_t
tag_music_crc(const LhTagParams & p, const unsigned char *bytes, long long n, LhTagLds & lds)
{
    int const tid = (int) threadIdx.x, lane = lh_lane(), wave = lh_wave_id();
    /* (places count from the stream's first byte, `lead' bytes behind a 16-byte boundary of memory; the body ends at the
     * last such boundary in front of the stream's end) */
    long long const lead = (long long) ((uintptr_t) bytes & (LH_TAG_PIECE - 1));
    long long const body = ((lead + n) & ~(long long) (LH_TAG_PIECE - 1)) - lead;
    long long const rows = body > 0 ? (body + lead + LH_TAG_ROW - 1) / LH_TAG_ROW : 0;
    long long q = body - rows * LH_TAG_ROW + (long long) tid * LH_TAG_PIECE;
    uint32_t acc = 0;
    LhTagPiece cur = { {0, 0, 0, 0} };
    if (rows > 0)
        cur = tag_piece(bytes, q, body);
    for (long long r = 0; r < rows; r++) {
        /* (the next piece is on its way while this one is worked through) */
        LhTagPiece next = { {0, 0, 0, 0} };
        if (r + 1 < rows)
            next = tag_piece(bytes, q + LH_TAG_ROW, body);
        acc = lh_tag_crc_advance(acc, p.adv[LH_TAG_ADV_GAP]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            acc = lh_tag_crc_byte(acc, cur.w[k]);
            acc = lh_tag_crc_byte(acc, cur.w[k] >> 8);
            acc = lh_tag_crc_byte(acc, cur.w[k] >> 16);
            acc = lh_tag_crc_byte(acc, cur.w[k] >> 24);
        }
        cur = next;
        q += LH_TAG_ROW;
    }
    /* the lanes of a wave, pairwise: the lower half's CRC moves on over the upper half's bytes */
#pragma unroll
    for (int j = 0; j < LH_TAG_ADV_WAVE; j++) {
        int const d = 1 << j;
        uint32_t const other = lh_shfl_u32(acc, lane ^ d);
        uint32_t const lower = (lane & d) ? other : acc, upper = (lane & d) ? acc : other;
        acc = lh_tag_crc_advance(lower, p.adv[j]) ^ upper;
    }
    if (lane == 0)
        lds.wave_crc[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        acc = lds.wave_crc[0];
        for (int k = 1; k < LH_TAG_WAVES; k++)
            acc = lh_tag_crc_advance(acc, p.adv[LH_TAG_ADV_WAVE]) ^ lds.wave_crc[k];
        for (long long a = body > 0 ? body : 0; a < n; a++)
            acc = lh_tag_crc_byte(acc, bytes[a]);
    }
    return acc;
}

/* B, for frames n0 .. n0 + n - 1 of a stream whose frames in front of them add up to sum0: the records fr[0 .. n) add
 * their samples to the bag in LDS at sampling distance w (that of n0 + n frames); all lanes of the workgroup call it and
 * get the new sum */
LH_TAG_FN int
tag_bag_add(const LhTagParams & p, const LhFrameOut * fr, int n, int n0, int sum0, int w, LhTagLds & lds)
{
    int const tid = (int) threadIdx.x, lane = lh_lane(), wave = lh_wave_id();
    int     running = sum0;
    for (int t0 = 0; t0 < n; t0 += LH_TAG_NT) {
        int const f = t0 + tid, g = n0 + f;
        uint32_t v = f < n ? (uint32_t) p.kbps[fr[f].bitrate_index & 15] : 0u;
        int     base = running, tile = 0;
        for (int d = 1; d < 64; d += d) {
            uint32_t const below = lh_shfl_u32(v, lane - d);
            if (lane >= d)
                v += below;
        }
        if (lane == 63)
            lds.wave_sum[wave] = (int) v;
        __syncthreads();
        for (int k = 0; k < LH_TAG_WAVES; k++) {
            if (k < wave)
                base += lds.wave_sum[k];
            tile += lds.wave_sum[k];
        }
        if (f < n && (g + 1) % w == 0 && (g + 1) / w - 1 < LH_TAG_BAG_SIZE)
            lds.bag[(g + 1) / w - 1] = base + (int) v;
        running += tile;
        __syncthreads();
    }
    return running;
}

/* B: what n calls of lh_tag_add_frame leave -- the bag in LDS, its fill, the sampling distance and the sum -- from the
 * bit-rate indices of the records fr[0 .. n); all lanes of the workgroup call it and get the three figures */
LH_TAG_FN void
tag_bag(const LhTagParams & p, const LhFrameOut * fr, int n, LhTagLds & lds, int *pos, int *want, int *sum)
{
    int const w = lh_tag_want(n);
    *sum = tag_bag_add(p, fr, n, 0, 0, w, lds);
    *pos = n / w;
    *want = w;
}

/* C: the frame in LDS from the bag there -- the template, the seek table's 99 entries a lane each, the other fields in lane
 * 0 (which holds the music CRC) --, and out to `tag'.  info: the stream's own info byte (lh_tag.h: lh_tag_pad_info), which
 * takes the template's place before the CRCs are taken, or -1 */
LH_TAG_FN void
tag_frame_out(const LhTagParams & p, const unsigned char *tmpl, int pos, int sum, uint32_t nf, long long n, uint32_t crc, int enc_padding,
              int info, int last_mode_ext, unsigned char *tag, LhTagLds & lds)
{
    int const tid = (int) threadIdx.x;
    for (int i = tid; i < p.total; i += LH_TAG_NT)
        lds.frame[i] = tmpl[i];
    __syncthreads();
    if (tid >= 1 && tid < 100)
        lds.frame[p.at + LH_TAG_AT_TOC + tid] = lh_tag_toc_entry(tid, lds.bag, pos, sum);
    if (tid == 0 && info >= 0)
        lds.frame[p.at + LH_TAG_AT_EXT + LH_TAG_EXT_INFO] = (unsigned char) info;
    __syncthreads();
    if (tid == 0)
        lh_tag_finish_fields(lds.frame, p.at, p.sideinfo_len, p.error_protection, nf, (uint32_t) (n + p.total), crc, enc_padding,
                             last_mode_ext);
    __syncthreads();
    for (int i = tid; i < p.total; i += LH_TAG_NT)
        tag[i] = lds.frame[i];
}

/* one stream: its tag frame to `tag' (p.total bytes), from the n audio bytes at `audio' and its nf frames' records */
LH_TAG_FN void
tag_stream(const LhTagParams & p, const unsigned char *audio, long long n, const LhFrameOut * fr, int nf, int enc_padding,
           const unsigned char *tmpl, unsigned char *tag, LhTagLds & lds)
{
    int const tid = (int) threadIdx.x;
    int     pos, want, sum;
    if (nf <= 0) {
        for (int i = tid; i < p.total; i += LH_TAG_NT)
            tag[i] = 0;
        return;
    }
    uint32_t const crc = tag_music_crc(p, audio, n, lds);
    tag_bag(p, fr, nf, lds, &pos, &want, &sum);
    tag_frame_out(p, tmpl, pos, sum, (uint32_t) nf, n, crc, enc_padding, -1, fr[nf - 1].mode_ext, tag, lds);
}

/* grid: one workgroup per stream.  descs / states: the launch's; out: its records; bytes: the pool, in which stream s's
 * audio starts at descs[s].bytes_base with p.total bytes of room for the tag in front; padding: the end padding per stream */
__global__ void
__launch_bounds__(LH_TAG_NT)
lh_tag_kernel(LhTagParams p, const LhStreamDesc * descs, const LhStreamState * states, const LhFrameOut * out, unsigned char *bytes,
              const unsigned char *tmpl, const int *padding, int nstreams)
{
    __shared__ LhTagLds lds;
    int const s = (int) blockIdx.x;
    if (s >= nstreams)
        return;
    long long const base = descs[s].bytes_base, cap = descs[s].bytes_cap, n = states[s].em_next_header;
    int     nf = descs[s].frame_end - descs[s].frame_begin;
    /* (no tag for a stream whose packer gave up, or whose length is not one its slice could hold) */
    if (states[s].status != 0 || n < 0 || n > cap)
        nf = 0;
    tag_stream(p, bytes + base, n, out + descs[s].out_index, nf, padding[s], tmpl, bytes + base - p.total, lds);
}

/* One stream of an incremental batch, one round: the carry *c moved on over the bytes [c->crc_upto, upto) of `slice' and the
 * round's nf records, and behind the flush (`final') the frame to `tag'.  Nothing of the slice at or behind `upto' is read:
 * the reservoir still back-fills there.  bad_now: the round found the stream with a status or an impossible position.
 * pad_entry: the stream's entry of the padding table -- its end padding, and its own info byte if it has one (lh_tag.h). */
LH_TAG_FN void
tag_resume(const LhTagParams & p, const LhTagPow * pw, const unsigned char *slice, long long upto, int bad_now, const LhFrameOut * fr, int nf,
           int final, int pad_entry, const unsigned char *tmpl, LhTagCarry * c, unsigned char *tag, LhTagLds & lds)
{
    int const tid = (int) threadIdx.x;
    long long const from = c->crc_upto;
    int const n0 = c->frames, want0 = c->want > 0 ? c->want : 1, pos0 = c->pos, sum0 = c->sum;
    /* (a carry that is not one this kernel left -- its bag's fill and distance not those of its frame count -- counts as bad
     * too: the bag is indexed by them) */
    int const bad = c->bad | bad_now | (upto < from) | (from < 0) | (n0 < 0) | (want0 != lh_tag_want(n0)) | (pos0 != n0 / want0);
    int     mode_ext = c->mode_ext;
    uint32_t crc = c->crc;
    /* (every lane has the carry before lane 0 writes it) */
    __syncthreads();
    if (bad) {
        if (tid == 0)
            c->bad = 1;
        if (final)
            for (int i = tid; i < p.total; i += LH_TAG_NT)
                tag[i] = 0;
        return;
    }
    long long const nb = upto - from;
    if (nb == 0 && nf <= 0 && !final)
        return;
    /* A: the new bytes' CRC from 0, the carried one moved on over as many zeros */
    if (nb > 0) {
        uint32_t const fresh = tag_music_crc(p, slice + from, nb, lds);
        if (tid == 0)
            crc = lh_tag_crc_advance_by(crc, pw, nb) ^ fresh;
    }
    /* B: the carried bag into LDS -- at the sampling distance of all frames so far, which keeps every (want1 / want0)-th of
     * its samples --, then the round's frames */
    int const n1 = n0 + (nf > 0 ? nf : 0), want1 = lh_tag_want(n1), pos1 = n1 / want1;
    int const step = want1 / want0, keep = pos0 / step;
    for (int j = tid; j < keep; j += LH_TAG_NT)
        lds.bag[j] = c->bag[(j + 1) * step - 1];
    __syncthreads();
    int const sum1 = tag_bag_add(p, fr, nf, n0, sum0, want1, lds);
    if (nf > 0) {
        mode_ext = fr[nf - 1].mode_ext;
        for (int j = tid; j < pos1; j += LH_TAG_NT)
            c->bag[j] = lds.bag[j];
    }
    if (tid == 0) {
        c->crc_upto = upto;
        c->crc = crc;
        c->frames = n1;
        c->want = want1;
        c->pos = pos1;
        c->sum = sum1;
        c->mode_ext = mode_ext;
    }
    /* D */
    if (!final)
        return;
    if (n1 <= 0) {
        for (int i = tid; i < p.total; i += LH_TAG_NT)
            tag[i] = 0;
        return;
    }
    tag_frame_out(p, tmpl, pos1, sum1, (uint32_t) n1, upto, crc, lh_tag_pad_padding(pad_entry), lh_tag_pad_info(pad_entry), mode_ext, tag, lds);
}

/* grid: one workgroup per stream, behind a round's drain.  descs / states: the round's; rows: the drain's table (upto: the
 * position up to which the slice is final); out: the round's records; pool: the byte pool; carry: a record per stream;
 * tags: p.total bytes per stream, written behind the flush only; padding: the end padding per stream, read then.  A stream
 * is behind its flush in the round in which it ends: its descriptor says flush and names frames (a slot whose stream ended
 * in an earlier round keeps the flag without frames: its frame has been made and is left alone), or `final' says it of all
 * streams. */
__global__ void
__launch_bounds__(LH_TAG_NT)
lh_tag_resume_kernel(LhTagParams p, const LhTagPow * pw, const LhStreamDesc * descs, const LhStreamState * states, const LhDrainRow * rows,
                     const LhFrameOut * out, const unsigned char *pool, const unsigned char *tmpl, const int *padding, LhTagCarry * carry,
                     unsigned char *tags, int final, int nstreams)
{
    __shared__ LhTagLds lds;
    int const s = (int) blockIdx.x;
    if (s >= nstreams)
        return;
    long long const upto = rows[s].upto;
    int const nf = descs[s].frame_end - descs[s].frame_begin;
    int const bad = states[s].status != 0 || rows[s].status != 0 || upto < 0 || upto > descs[s].bytes_cap;
    int const ends = final || (descs[s].flush && nf > 0);
    tag_resume(p, pw, pool + descs[s].bytes_base, upto, bad, out + descs[s].out_index, nf, ends, ends ? padding[s] : 0, tmpl, &carry[s],
               tags + (long long) s * p.total, lds);
}

#ifndef LH_EMU
/* The tag launch of an incremental batch's round.  Returns a hipError_t. */
extern "C" int
lh_launch_tag_resume(const LhTagParams * p, const LhTagPow * pw, const LhStreamDesc * descs, const LhStreamState * states,
                     const LhDrainRow * rows, const LhFrameOut * out, const unsigned char *pool, const unsigned char *tmpl, const int *padding,
                     LhTagCarry * carry, unsigned char *tags, int final, int nstreams, void *stream)
{
    if (nstreams <= 0)
        return 0;
    if (p->total < 1 || p->total > LH_TAG_MAX_FRAME || p->at < 4 || p->at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC + 2 > p->total)
        return (int) hipErrorInvalidValue;
    hipLaunchKernelGGL(lh_tag_resume_kernel, dim3((unsigned) nstreams), dim3(LH_TAG_NT), 0, (hipStream_t) stream, *p, pw, descs, states, rows,
                       out, pool, tmpl, padding, carry, tags, final, nstreams);
    return (int) hipGetLastError();
}

/* Returns a hipError_t. */
extern "C" int
lh_launch_tag(const LhTagParams * p, const LhStreamDesc * descs, const LhStreamState * states, const LhFrameOut * out, unsigned char *bytes,
              const unsigned char *tmpl, const int *padding, int nstreams, void *stream)
{
    if (nstreams <= 0)
        return 0;
    if (p->total < 1 || p->total > LH_TAG_MAX_FRAME || p->at < 4 || p->at + LH_TAG_AT_EXT + LH_TAG_EXT_CRC + 2 > p->total)
        return (int) hipErrorInvalidValue;
    hipLaunchKernelGGL(lh_tag_kernel, dim3((unsigned) nstreams), dim3(LH_TAG_NT), 0, (hipStream_t) stream, *p, descs, states, out, bytes,
                       tmpl, padding, nstreams);
    return (int) hipGetLastError();
}
#else
/* TEST ENTRY POINTS (tests/hipemu_tag): the kernel's parts and the kernel under the fiber emulator */
extern "C" int
lh_emu_tag_crc(const LhTagParams * params, const unsigned char *bytes, long long n, unsigned *crc)
{
    LhTagParams const p = *params;
    hipemu_dim3 grid = { 1, 1, 1 }, block = { LH_TAG_NT, 1, 1 };
    hipemu_run(grid, block,[=] () {
               __shared__ LhTagLds lds;
               uint32_t const c = tag_music_crc(p, bytes, n, lds);
               if (threadIdx.x == 0)
                   *crc = c;
               }
    );
    return 0;
}

/* bag: LH_TAG_BAG_SIZE entries, of which pos are written; psw: pos, want, sum */
extern "C" int
lh_emu_tag_bag(const LhTagParams * params, const signed char *bitrate_index, int n, int *bag, int *psw)
{
    LhTagParams const p = *params;
    std::vector < LhFrameOut > fr((size_t) (n > 0 ? n : 1));
    hipemu_dim3 grid = { 1, 1, 1 }, block = { LH_TAG_NT, 1, 1 };
    for (int f = 0; f < n; f++)
        fr[(size_t) f].bitrate_index = bitrate_index[f];
    const LhFrameOut *const frames = fr.data();
    hipemu_run(grid, block,[=] () {
               __shared__ LhTagLds lds;
               int     pos, want, sum;
               tag_bag(p, frames, n, lds, &pos, &want, &sum);
               if (threadIdx.x == 0) {
                   psw[0] = pos;
                   psw[1] = want;
                   psw[2] = sum;
                   for (int j = 0; j < pos; j++)
                       bag[j] = lds.bag[j];
               }
               }
    );
    return 0;
}

/* the host's gain patch of lh_tag.h, as this library compiled it */
extern "C" void
lh_emu_tag_patch_gain(unsigned char *frame, int at, int radio_gain)
{
    lh_tag_patch_gain(frame, at, radio_gain);
}

/* the kernel over nstreams streams.  Per stream: audio bytes, status and frame count as the encode kernel would leave
 * them, the end padding, the last frame's mode extension; bitrate_index: the streams' lists one behind the other;
 * bytes_base: where each stream's audio starts in `pool' (the tag goes in front) */
extern "C" int
lh_emu_tag(const LhTagParams * params, const unsigned char *tmpl, int nstreams, const long long *nbytes, const int *status,
           const int *nframes, const int *padding, const int *last_mode_ext, const signed char *bitrate_index,
           const long long *bytes_base, const long long *bytes_cap, unsigned char *pool)
{
    LhTagParams const p = *params;
    std::vector < LhStreamDesc > descs((size_t) nstreams);
    std::vector < LhStreamState > states((size_t) nstreams);
    long long total = 0;
    for (int s = 0; s < nstreams; s++)
        total += nframes[s];
    std::vector < LhFrameOut > fr((size_t) (total > 0 ? total : 1));
    total = 0;
    for (int s = 0; s < nstreams; s++) {
        memset(&descs[(size_t) s], 0, sizeof(LhStreamDesc));
        memset(&states[(size_t) s], 0, sizeof(LhStreamState));
        descs[(size_t) s].out_index = total;
        descs[(size_t) s].frame_end = nframes[s];
        descs[(size_t) s].bytes_base = bytes_base[s];
        descs[(size_t) s].bytes_cap = bytes_cap[s];
        states[(size_t) s].status = status[s];
        states[(size_t) s].em_next_header = nbytes[s];
        for (int f = 0; f < nframes[s]; f++) {
            fr[(size_t) (total + f)].bitrate_index = bitrate_index[total + f];
            fr[(size_t) (total + f)].mode_ext = (int8_t) (f == nframes[s] - 1 ? last_mode_ext[s] : 3 - last_mode_ext[s]);
        }
        total += nframes[s];
    }
    const LhStreamDesc *const d = descs.data();
    const LhStreamState *const st = states.data();
    const LhFrameOut *const frames = fr.data();
    hipemu_dim3 grid = { (unsigned) nstreams, 1, 1 }, block = { LH_TAG_NT, 1, 1 };
    if (nstreams <= 0)
        return 0;
    hipemu_run(grid, block,[=] () {
               lh_tag_kernel(p, d, st, frames, pool, tmpl, padding, nstreams);
               }
    );
    return 0;
}

/* TEST ENTRY POINTS (tests/hipemu_tag_inc): one round of lh_tag_resume_kernel over nstreams streams.  Per stream: the
 * position the drain found (upto), the status of the packer and of the drain's row, the round's frame count, the end
 * padding, the mode extension of the round's last frame; bitrate_index: the round's lists one behind the other; carry:
 * nstreams records the caller keeps from round to round; tags: nstreams rows of params->total bytes */
static int
emu_tag_resume(const LhTagParams * params, const LhTagPow * pw, const unsigned char *tmpl, int nstreams, const long long *upto,
               const int *status, const int *row_status, const int *nframes, const int *padding, const int *last_mode_ext,
               const signed char *bitrate_index, const long long *bytes_base, const long long *bytes_cap, const unsigned char *pool,
               LhTagCarry * carry, unsigned char *tags, int final, const int *flush)
{
    LhTagParams const p = *params;
    std::vector < LhStreamDesc > descs((size_t) (nstreams > 0 ? nstreams : 1));
    std::vector < LhStreamState > states(descs.size());
    std::vector < LhDrainRow > rows(descs.size() + 1);
    long long total = 0;
    for (int s = 0; s < nstreams; s++)
        total += nframes[s];
    std::vector < LhFrameOut > fr((size_t) (total > 0 ? total : 1));
    total = 0;
    for (int s = 0; s < nstreams; s++) {
        memset(&descs[(size_t) s], 0, sizeof(LhStreamDesc));
        memset(&states[(size_t) s], 0, sizeof(LhStreamState));
        memset(&rows[(size_t) s], 0, sizeof(LhDrainRow));
        descs[(size_t) s].out_index = total;
        descs[(size_t) s].frame_begin = 5;      /* (the records count from the round's first frame, whatever its number) */
        descs[(size_t) s].frame_end = 5 + nframes[s];
        descs[(size_t) s].bytes_base = bytes_base[s];
        descs[(size_t) s].bytes_cap = bytes_cap[s];
        descs[(size_t) s].flush = flush ? flush[s] : 0;
        states[(size_t) s].status = status[s];
        rows[(size_t) s].status = row_status[s];
        rows[(size_t) s].upto = upto[s];
        for (int f = 0; f < nframes[s]; f++) {
            fr[(size_t) (total + f)].bitrate_index = bitrate_index[total + f];
            fr[(size_t) (total + f)].mode_ext = (int8_t) (f == nframes[s] - 1 ? last_mode_ext[s] : 3 - last_mode_ext[s]);
        }
        total += nframes[s];
    }
    const LhStreamDesc *const d = descs.data();
    const LhStreamState *const st = states.data();
    const LhDrainRow *const rw = rows.data();
    const LhFrameOut *const frames = fr.data();
    hipemu_dim3 grid = { (unsigned) nstreams, 1, 1 }, block = { LH_TAG_NT, 1, 1 };
    if (nstreams <= 0)
        return 0;
    hipemu_run(grid, block,[=] () {
               lh_tag_resume_kernel(p, pw, d, st, rw, frames, pool, tmpl, padding, carry, tags, final, nstreams);
               }
    );
    return 0;
}

extern "C" int
lh_emu_tag_resume(const LhTagParams * params, const LhTagPow * pw, const unsigned char *tmpl, int nstreams, const long long *upto,
                  const int *status, const int *row_status, const int *nframes, const int *padding, const int *last_mode_ext,
                  const signed char *bitrate_index, const long long *bytes_base, const long long *bytes_cap, const unsigned char *pool,
                  LhTagCarry * carry, unsigned char *tags, int final)
{
    return emu_tag_resume(params, pw, tmpl, nstreams, upto, status, row_status, nframes, padding, last_mode_ext, bitrate_index, bytes_base,
                          bytes_cap, pool, carry, tags, final, nullptr);
}

/* (tests/hipemu_slots) the same round with the flush per stream, flush[s] = LhStreamDesc.flush of stream s */
extern "C" int
lh_emu_tag_resume_slots(const LhTagParams * params, const LhTagPow * pw, const unsigned char *tmpl, int nstreams, const long long *upto,
                        const int *status, const int *row_status, const int *nframes, const int *padding, const int *last_mode_ext,
                        const signed char *bitrate_index, const long long *bytes_base, const long long *bytes_cap,
                        const unsigned char *pool, LhTagCarry * carry, unsigned char *tags, int final, const int *flush)
{
    return emu_tag_resume(params, pw, tmpl, nstreams, upto, status, row_status, nframes, padding, last_mode_ext, bitrate_index, bytes_base,
                          bytes_cap, pool, carry, tags, final, flush);
}

/* a CRC moved on over n zero bytes through the table, as this library compiled lh_tag.h */
extern "C" unsigned
lh_emu_tag_advance_by(unsigned crc, const LhTagPow * pw, long long n)
{
    return lh_tag_crc_advance_by(crc, pw, n);
}

extern "C" int
lh_emu_tag_sizeof_carry(void)
{
    return (int) sizeof(LhTagCarry);
}
#endif
