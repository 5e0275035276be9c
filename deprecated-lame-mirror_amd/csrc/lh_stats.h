/*
 * lh_stats.h -- the statistics the reference keeps per stream (updateStats, reference encoder.c:156-184, read through
 * lame_bitrate_hist, lame_stereo_mode_hist, lame_bitrate_stereo_mode_hist, lame_block_type_hist and
 * lame_bitrate_block_type_hist): how one frame's LhFrameOut record is counted, ONE text for the handle API
 * (lh_api.cpp), for a batch's kernel (lh_stats.hip: the same lines compiled for the device, adding into LDS) and for the
 * host twin the tests compare the kernel with.  Integers only.
 *
 * LhStatCarry is the reference's pair of tables: mode[bitrate index | 15 = all][mode extension 0..3 | 4 = frames] is
 * bitrate_channelmode_hist, block[bitrate index | 15 = all][block type 0..3 | 4 = mixed | 5 = granules] is
 * bitrate_blocktype_hist.  A frame counts once into `mode' -- and by its mode extension when the stream has two
 * channels -- and once per granule and channel that the stream has into `block': mode_gr granules (2, MPEG-2 / 2.5: 1),
 * `channels' channels.  Nothing of a record's other granules and channels is read: the encode kernel leaves them as the
 * pool was.
 *
 * A frame is taken in two steps, so that a kernel can have the reads of several frames in flight before it adds any of
 * them: lh_stats_key reads the record (its tail and up to four granules' two bytes) into one word, lh_stats_add counts
 * the word.  LH_STATS_ADD(p) is how a bin goes up by one: ++*p unless the includer says otherwise.
 */
#ifndef LH_STATS_H
#define LH_STATS_H

#include <stdint.h>
#include "lamehip_types.h"

#ifndef LH_STATS_FN
#define LH_STATS_FN static inline
#endif
#ifndef LH_STATS_ADD
#define LH_STATS_ADD(p) (++*(p))
#endif

#define LH_STATS_WORDS 176      /* ints of an LhStatCarry */

typedef struct LhStatCarry {
    int     mode[16][5];
    int     block[16][6];
} LhStatCarry;

/* a frame's key: bits 0..3 the bit rate index, 4..5 the mode extension, then three bits per (granule, channel) at
 * 6 + 3 * (2 * gr + ch): the bin of `block' (0..4), or 7 for a granule or channel the stream does not have */
#define LH_STATS_NONE 7u

LH_STATS_FN uint32_t
lh_stats_key(const LhFrameOut * fo, int channels, int mode_gr)
{
    uint32_t key = ((uint32_t) fo->bitrate_index & 15u) | (((uint32_t) fo->mode_ext & 3u) << 4);
    int     gr, ch;
    for (gr = 0; gr < 2; gr++)
        for (ch = 0; ch < 2; ch++) {
            uint32_t bt = LH_STATS_NONE;
            if (gr < mode_gr && ch < channels)
                bt = fo->gr[gr][ch].mixed_block_flag ? 4u : ((uint32_t) fo->gr[gr][ch].block_type & 3u);
            key |= bt << (6 + 3 * (2 * gr + ch));
        }
    return key;
}

LH_STATS_FN void
lh_stats_add(LhStatCarry * c, uint32_t key, int channels)
{
    int const bi = (int) (key & 15u), me = (int) ((key >> 4) & 3u);
    int     k;
    LH_STATS_ADD(&c->mode[bi][4]);
    LH_STATS_ADD(&c->mode[15][4]);
    if (channels == 2) {
        LH_STATS_ADD(&c->mode[bi][me]);
        LH_STATS_ADD(&c->mode[15][me]);
    }
    for (k = 0; k < 4; k++) {
        int const bt = (int) ((key >> (6 + 3 * k)) & 7u);
        if (bt != (int) LH_STATS_NONE) {
            LH_STATS_ADD(&c->block[bi][bt]);
            LH_STATS_ADD(&c->block[bi][5]);
            LH_STATS_ADD(&c->block[15][bt]);
            LH_STATS_ADD(&c->block[15][5]);
        }
    }
}

/* one frame, as the handle API and the host twin count it */
LH_STATS_FN void
lh_stats_count_frame(LhStatCarry * c, const LhFrameOut * fo, int channels, int mode_gr)
{
    lh_stats_add(c, lh_stats_key(fo, channels, mode_gr), channels);
}

#endif /* LH_STATS_H */
