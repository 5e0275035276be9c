/*
 * lh_drain.h -- the records of the drain kernels (lh_drain.hip) of an incremental batch that packs on the device
 * (lamehip_batch_set_incremental_packing), and the host's half of a round's drain in plain C: the bound on what a stream
 * may have finished and the table of tiles the gather's grid is made of.  ONE text for the library (lh_batch.cpp), the
 * emulator's twin and the stand-alone check (tests/hipemu_drain).
 *
 * A round's drain answers, per stream, "which bytes of the slice are final" -- the position P the reference's putbits has
 * reached: the packer's cursor, or the start of a queued header the frame's main data ended on exactly (the reference
 * writes a header only with the next bit behind it, the device packer steps over it at once), or, behind the flush, the
 * end of the last frame -- and gathers [drained, P) of every slice into one round buffer, every stream on a 16-byte
 * boundary, which comes home with one copy.
 */
#ifndef LH_DRAIN_H
#define LH_DRAIN_H

#include <stdint.h>

#define LH_DR_NT 256            /* lanes of a workgroup, all three kernels */
#define LH_DR_PIECE 16          /* bytes a lane moves at a time */
#define LH_DR_PIECES 2          /* pieces per lane and tile */
#define LH_DR_TILE (LH_DR_NT * LH_DR_PIECE * LH_DR_PIECES)      /* bytes of a stream one workgroup of the gather takes */

typedef struct LhDrainParams {
    int     sideinfo_len;
    int     frame_factor;       /* (version + 1) * 72000: a frame is frame_factor * kbps / samplerate bytes + the padding bit */
    int     samplerate;
    int     final;              /* every stream is behind the flush: P is the end of the last frame (one stream: LhStreamDesc.flush) */
    int16_t kbps[16];           /* the MPEG version's bit rates by index */
} LhDrainParams;

/* what comes home per stream, in front of the bytes; row [nstreams] holds the round's total in `off' */
typedef struct LhDrainRow {
    long long off;              /* where the stream's bytes start in the round buffer (a multiple of LH_DR_PIECE) */
    long long n;                /* how many there are: P - drained */
    long long upto;             /* P */
    long long next;             /* LhStreamState.em_next_header: where the stream's next frame will start */
    int     status;             /* LhStreamState.status; bit 16: P lies outside the slice or in front of `drained' */
    int     pad;
} LhDrainRow;

#define LH_DR_STATUS_RANGE 16

typedef struct LhDrainTile {
    int     stream;
    int     tile;               /* bytes [tile * LH_DR_TILE, (tile + 1) * LH_DR_TILE) of the stream's range */
} LhDrainTile;

/* the most a stream can have finished and not handed out behind a round: its frames ended at `known' when the last table
 * came home (LhDrainRow.next; 0 at first), the round adds `frames' frames of at most `frame_max' bytes, all inside a slice
 * of `cap' bytes, and the host has handed out `drained' bytes */
static inline long long
lh_drain_bound(long long known, long long frames, long long frame_max, long long cap, long long drained)
{
    long long hi = (known > 0 ? known : 0) + (frames > 0 && frame_max > 0 ? frames * frame_max : 0);
    if (hi > cap)
        hi = cap;
    return hi > drained ? hi - drained : 0;
}

/* the tiles of a round: stream after stream, every stream's bound cut into LH_DR_TILE bytes.  Returns their number;
 * writes the first `room' of them (call it with room = 0 for the count).  *padded: the bytes of a round buffer that holds
 * every stream's bound on a boundary of its own. */
static inline long long
lh_drain_tiles(const long long *bound, int nstreams, LhDrainTile * tiles, long long room, long long *padded)
{
    long long n = 0, bytes = 0;
    int     s;
    for (s = 0; s < nstreams; s++) {
        long long const b = bound[s] > 0 ? bound[s] : 0;
        long long const nt = (b + LH_DR_TILE - 1) / LH_DR_TILE;
        long long t;
        for (t = 0; t < nt; t++, n++)
            if (n < room) {
                tiles[n].stream = s;
                tiles[n].tile = (int) t;
            }
        bytes += (b + LH_DR_PIECE - 1) / LH_DR_PIECE * LH_DR_PIECE;
    }
    if (padded)
        *padded = bytes;
    return n;
}

#endif
