/*
 * lh_drain.hip -- the drain of an incremental batch that packs on the device (gfx950): behind a round's encode launch,
 * three small launches find what every stream has finished, lay the streams out in one round buffer and gather them, so
 * that the round's bytes come home with one copy of exactly their size (lh_drain.h; lh_batch.cpp: batch_drain_launch).
 *   lh_drain_pos_kernel     a lane per stream: the position P up to which the slice is final.  P is the packer's cursor
 *      -- unless the cursor stands one side-information length behind the start of a header that is already out: then the
 *      frame's main data ended on that header exactly, the packer (lh_emit_pos) stepped over it at once, and the reference,
 *      which writes a header only with the next bit behind it, has not written it yet: P is the header's start.  Behind
 *      the flush -- of the stream: LhStreamDesc.flush, or of all of them: LhDrainParams.final -- P is the end of the last
 *      frame.  Whether a header starts at cursor - sideinfo_len is found by walking:
 *      every stream carries the start of a header in HBM (`carry', 0 at first), and the lane moves it on frame by frame --
 *      a frame's length stands in its header's third byte, bit-rate index and padding bit, which the packer has written for
 *      every header in front of em_next_header -- while the next start does not pass the cursor.
 *   lh_drain_scan_kernel    one workgroup: the exclusive prefix sum of the streams' byte counts, each rounded up to
 *      LH_DR_PIECE, over tiles of LH_DR_NT streams -- shuffles inside a wave, LDS across the waves, a running base from
 *      tile to tile.  Row [nstreams] gets the total.
 *   lh_drain_gather_kernel  a workgroup per tile of the host's table (LH_DR_TILE bytes of one stream's bound; a tile
 *      behind the stream's count leaves at once).  A lane moves LH_DR_PIECE bytes at a time: the destination is on a
 *      16-byte boundary by the layout, the source anywhere, so a piece is two aligned 16-byte loads, the eight words shifted
 *      by the source's residue (the same for the whole stream, so wave-uniform), and one aligned 16-byte store.  The 64
 *      lanes of a wave load and store 1 KB side by side.  A piece whose loads would reach in front of `drained' or
 *      behind P, or whose store would reach behind the stream's count, goes byte by byte, inside the range only.
 * Bandwidth-bound, and small: a round of 256 streams x 1 s at 128 kb/s gathers 4 MB.
 */
#include <stdint.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_DR_FN static inline
#else
#include <hip/hip_runtime.h>
#define LH_DR_FN static __device__ __forceinline__
#endif
#include "lh_wave.h"
#include "lh_device.h"
#include "lh_drain.h"

#define LH_DR_WAVES (LH_DR_NT / 64)

typedef uint32_t lh_dr_v4 __attribute__((vector_size(16)));

/* P of one stream (see above); final: the stream is behind its flush; *carry: the header start the walk has reached */
LH_DR_FN long long
drain_position(const LhDrainParams & p, int final, const LhStreamState * st, const unsigned char *slice, long long cap, long long *carry)
{
    long long const next = st->em_next_header, cursor = st->em_cursor, target = cursor - p.sideinfo_len;
    long long h = *carry;
    if (final)
        return next;
    /* (a header at h is in the slice when h lies in front of em_next_header; its frame ends at the next one's start) */
    while (h >= 0 && h < target && h < next && h + 4 <= cap) {
        unsigned const b2 = slice[h + 2];
        long long const len = (long long) p.frame_factor * p.kbps[b2 >> 4] / p.samplerate + ((b2 >> 1) & 1u);
        if (len <= 0 || h + len > target)
            break;
        h += len;
    }
    *carry = h;
    return (h == target && h < next) ? h : cursor;
}

/* grid: a lane per stream.  descs: the round's (bytes_base, bytes_cap, flush); drained: what the host has handed out per
 * stream.  A stream is behind its flush when the round's descriptor says so -- it ends in this round, or it ended in an
 * earlier one and its slot has not been restarted: no frames then, and the same P round after round -- or when p.final
 * says it of all of them. */
__global__ void
__launch_bounds__(LH_DR_NT)
lh_drain_pos_kernel(LhDrainParams p, const LhStreamDesc * descs, const LhStreamState * states, const long long *drained,
                    long long *carry, const unsigned char *pool, LhDrainRow * rows, int nstreams)
{
    int const s = (int) (blockIdx.x * LH_DR_NT + threadIdx.x);
    if (s >= nstreams)
        return;
    long long const cap = descs[s].bytes_cap, from = drained[s];
    long long h = carry[s];
    long long const upto = drain_position(p, p.final | descs[s].flush, &states[s], pool + descs[s].bytes_base, cap, &h);
    int     status = states[s].status;
    carry[s] = h;
    if (upto < from || upto > cap || from < 0)
        status |= LH_DR_STATUS_RANGE;
    rows[s].off = 0;
    rows[s].n = status ? 0 : upto - from;
    rows[s].upto = upto;
    rows[s].next = states[s].em_next_header;
    rows[s].status = status;
    rows[s].pad = 0;
}

/* grid: ONE workgroup */
__global__ void
__launch_bounds__(LH_DR_NT)
lh_drain_scan_kernel(LhDrainRow * rows, int nstreams)
{
    __shared__ uint32_t wave_sum[LH_DR_WAVES];
    int const tid = (int) threadIdx.x, lane = lh_lane(), wave = lh_wave_id();
    long long running = 0;      /* pieces in front of the tile */
    for (int t0 = 0; t0 < nstreams; t0 += LH_DR_NT) {
        int const s = t0 + tid;
        uint32_t const mine = s < nstreams ? (uint32_t) ((rows[s].n + LH_DR_PIECE - 1) / LH_DR_PIECE) : 0u;
        uint32_t v = mine, base = 0, tile = 0;
        for (int d = 1; d < 64; d += d) {
            uint32_t const below = lh_shfl_u32(v, (lane - d) & 63);
            if (lane >= d)
                v += below;
        }
        if (lane == 63)
            wave_sum[wave] = v;
        __syncthreads();
        for (int k = 0; k < LH_DR_WAVES; k++) {
            if (k < wave)
                base += wave_sum[k];
            tile += wave_sum[k];
        }
        if (s < nstreams)
            rows[s].off = (running + base + v - mine) * LH_DR_PIECE;
        running += tile;
        __syncthreads();
    }
    if (tid == 0) {
        rows[nstreams].off = running * LH_DR_PIECE;
        rows[nstreams].n = 0;
        rows[nstreams].upto = 0;
        rows[nstreams].next = 0;
        rows[nstreams].status = 0;
        rows[nstreams].pad = 0;
    }
}

/* word k of the 16 bytes that start r bytes into the eight words (lo, hi); Q = r / 4, rb = r % 4 */
template < int Q > LH_DR_FN lh_dr_v4
drain_shift(lh_dr_v4 lo, lh_dr_v4 hi, unsigned rb)
{
    uint32_t const w[8] = { lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3] };
    lh_dr_v4 out;
#pragma unroll
    for (int k = 0; k < 4; k++)
        out[k] = rb ? (w[Q + k] >> (8 * rb)) | (w[Q + k + 1] << (32 - 8 * rb)) : w[Q + k];
    return out;
}

/* grid: a workgroup per tile */
__global__ void
__launch_bounds__(LH_DR_NT)
lh_drain_gather_kernel(const LhDrainTile * tiles, const LhStreamDesc * descs, const LhDrainRow * rows, const long long *drained,
                       const unsigned char *pool, unsigned char *round, long long round_cap)
{
    LhDrainTile const t = tiles[blockIdx.x];
    long long const n = rows[t.stream].n, lo = (long long) t.tile * LH_DR_TILE;
    /* (a stream that would not fit the round buffer is left out: the host, which sized the buffer from its bounds, sees it in
     * the table and refuses the round) */
    if (lo >= n || rows[t.stream].off + (n + LH_DR_PIECE - 1) / LH_DR_PIECE * LH_DR_PIECE > round_cap)
        return;
    const unsigned char *const src = pool + descs[t.stream].bytes_base + drained[t.stream];
    unsigned char *const dst = round + rows[t.stream].off;
    unsigned const r = (unsigned) ((uintptr_t) src & (LH_DR_PIECE - 1));
#pragma unroll
    for (int k = 0; k < LH_DR_PIECES; k++) {
        long long const i = lo + ((long long) k * LH_DR_NT + (long long) threadIdx.x) * LH_DR_PIECE;
        if (i >= n)
            continue;
        /* (the loads cover [i - r, i - r + 16), and 16 more when r != 0, of the stream's range [0, n)) */
        if (i + LH_DR_PIECE <= n && (r == 0 || (i >= (long long) r && i - r + 2 * LH_DR_PIECE <= n))) {
            const unsigned char *const a = src + i - r;
            lh_dr_v4 const v0 = *(const lh_dr_v4 *) __builtin_assume_aligned(a, LH_DR_PIECE);
            lh_dr_v4 out = v0;
            if (r != 0) {
                lh_dr_v4 const v1 = *(const lh_dr_v4 *) __builtin_assume_aligned(a + LH_DR_PIECE, LH_DR_PIECE);
                unsigned const rb = r & 3u;
                switch (r >> 2) {
                case 0:
                    out = drain_shift < 0 > (v0, v1, rb);
                    break;
                case 1:
                    out = drain_shift < 1 > (v0, v1, rb);
                    break;
                case 2:
                    out = drain_shift < 2 > (v0, v1, rb);
                    break;
                default:
                    out = drain_shift < 3 > (v0, v1, rb);
                    break;
                }
            }
            *(lh_dr_v4 *) __builtin_assume_aligned(dst + i, LH_DR_PIECE) = out;
        }
        else {
            for (int j = 0; j < LH_DR_PIECE; j++)
                if (i + j < n)
                    dst[i + j] = src[i + j];
        }
    }
}

#ifndef LH_EMU
/* The three launches of a round's drain on `stream'; rows: nstreams + 1 records.  Returns a hipError_t. */
extern "C" int
lh_launch_drain(const LhDrainParams * p, const LhStreamDesc * descs, const LhStreamState * states, const long long *drained,
                long long *carry, const unsigned char *pool, LhDrainRow * rows, int nstreams, const LhDrainTile * tiles, long long ntiles,
                unsigned char *round, long long round_cap, void *stream)
{
    if (nstreams <= 0)
        return 0;
    if (p->sideinfo_len < 1 || p->samplerate < 1 || p->frame_factor < 1 || ntiles < 0 || ntiles > 0x7fffffffll)
        return (int) hipErrorInvalidValue;
    hipLaunchKernelGGL(lh_drain_pos_kernel, dim3((unsigned) ((nstreams + LH_DR_NT - 1) / LH_DR_NT)), dim3(LH_DR_NT), 0, (hipStream_t) stream,
                       *p, descs, states, drained, carry, pool, rows, nstreams);
    hipLaunchKernelGGL(lh_drain_scan_kernel, dim3(1), dim3(LH_DR_NT), 0, (hipStream_t) stream, rows, nstreams);
    if (ntiles > 0)
        hipLaunchKernelGGL(lh_drain_gather_kernel, dim3((unsigned) ntiles), dim3(LH_DR_NT), 0, (hipStream_t) stream, tiles, descs, rows,
                           drained, pool, round, round_cap);
    return (int) hipGetLastError();
}
#else
/* TEST ENTRY POINT (tests/hipemu_drain): the three kernels under the fiber emulator, as lh_launch_drain queues them */
extern "C" int
lh_emu_drain(const LhDrainParams * params, const LhStreamDesc * descs, const LhStreamState * states, const long long *drained,
             long long *carry, const unsigned char *pool, LhDrainRow * rows, int nstreams, const LhDrainTile * tiles, long long ntiles,
             unsigned char *round, long long round_cap)
{
    LhDrainParams const p = *params;
    hipemu_dim3 block = { LH_DR_NT, 1, 1 };
    hipemu_dim3 g0 = { (unsigned) ((nstreams + LH_DR_NT - 1) / LH_DR_NT), 1, 1 }, g1 = { 1, 1, 1 }, g2 = { (unsigned) ntiles, 1, 1 };
    if (nstreams <= 0)
        return 0;
    hipemu_run(g0, block,[=] () {
               lh_drain_pos_kernel(p, descs, states, drained, carry, pool, rows, nstreams);
               }
    );
    hipemu_run(g1, block,[=] () {
               lh_drain_scan_kernel(rows, nstreams);
               }
    );
    if (ntiles > 0)
        hipemu_run(g2, block,[=] () {
                   lh_drain_gather_kernel(tiles, descs, rows, drained, pool, round, round_cap);
                   }
        );
    return 0;
}

/* the host's bound and tile table of lh_drain.h, as this library compiled them */
extern "C" long long
lh_emu_drain_bound(long long known, long long frames, long long frame_max, long long cap, long long drained)
{
    return lh_drain_bound(known, frames, frame_max, cap, drained);
}

extern "C" long long
lh_emu_drain_tiles(const long long *bound, int nstreams, LhDrainTile * tiles, long long room, long long *padded)
{
    return lh_drain_tiles(bound, nstreams, tiles, room, padded);
}

extern "C" int
lh_emu_drain_sizeof_state(void)
{
    return (int) sizeof(LhStreamState);
}
#endif
