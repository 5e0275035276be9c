/*
 * lh_stats.hip -- a batch's statistics on the device (gfx950): behind a launch's encode kernel, lh_stats_resume_kernel
 * counts the launch's LhFrameOut records where they lie in HBM into the five tables the reference keeps per stream
 * (lh_stats.h: LhStatCarry, and the rule for one frame, the text the handle API counts by), so that
 * lamehip_batch_get_statistics and the lamehip_batch_*_hist getters fetch 704 bytes per stream and no record.
 *   A workgroup of LH_STATS_NT lanes takes one stream and adds its frames [frame_begin, frame_end) -- the records
 *   out[out_index .. out_index + nf) -- to carry[s], which the host zeroes when the stream starts: a one-shot batch has one
 *   launch per stream, an incremental one a launch per round.
 *   A lane takes a frame at a time, LH_STATS_AHEAD frames per step: of each it reads the record's tail (bit rate index,
 *   mode extension) and the block type and mixed flag of the granules and channels the stream has, at most five places
 *   1224 bytes apart, into one word (lh_stats_key), all frames of the step before any of them is counted, so that the
 *   step's reads are in flight together.  Neighbouring lanes read records 4928 bytes apart: nothing coalesces, every read
 *   is a line of its own -- four 128-byte lines a frame of two granules and two channels, a tenth of the record.  Measured
 *   on an MI355X (profiles/batch_stats_bench.json): 0.29 ms for the 2.35 M frames of 1024 streams x 60 s, 1.5 times the
 *   time HBM needs for those lines; 0.0075 ms, a launch's own cost, for a round of 256 streams x 1 s.
 *   The words are counted into the workgroup's table in LDS (lh_stats_add through lh_lds_add: ds_add_u32 without a
 *   return value).  The lanes of a CBR stream meet in few bins; the two adds per frame that go to one place for every lane
 *   (all frames, all granules) the compiler folds into one add of the wave's count, and the others the LDS serialises: some
 *   ten adds per frame against five lines from HBM.  Behind a barrier the table's 176 words are added to the carry with
 *   plain loads and stores, a lane each; a stream has one workgroup, so nothing else writes them.
 *   A stream without frames in the launch returns before it touches anything.
 * Integers only; built with the flags of the other integer kernels.
 */
#include <stdint.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_STATS_FN static inline
#else
#include <hip/hip_runtime.h>
#define LH_STATS_FN static __device__ __forceinline__
#endif
#include "lh_wave.h"
#include "lh_device.h"
#define LH_STATS_ADD(p) lh_lds_add((p), 1)
#include "lh_stats.h"

#define LH_STATS_NT 256         /* lanes of a workgroup */
#define LH_STATS_AHEAD 4        /* frames a lane reads before it counts them */

/* grid: one workgroup per stream.  descs / out: the launch's descriptors and records; carry: a record per stream */
__global__ void
__launch_bounds__(LH_STATS_NT)
lh_stats_resume_kernel(const LhStreamDesc * descs, const LhFrameOut * out, int nstreams, int channels, int mode_gr, LhStatCarry * carry)
{
    __shared__ LhStatCarry bins;
    int const s = (int) blockIdx.x, tid = (int) threadIdx.x;
    if (s >= nstreams)
        return;
    int const nf = descs[s].frame_end - descs[s].frame_begin;
    if (nf <= 0)
        return;
    const LhFrameOut *const fr = out + descs[s].out_index;
    int    *const lds = &bins.mode[0][0];
    for (int i = tid; i < LH_STATS_WORDS; i += LH_STATS_NT)
        lds[i] = 0;
    __syncthreads();
    for (int f0 = tid; f0 < nf; f0 += LH_STATS_NT * LH_STATS_AHEAD) {
        uint32_t key[LH_STATS_AHEAD];
#pragma unroll
        for (int k = 0; k < LH_STATS_AHEAD; k++) {
            int const f = f0 + k * LH_STATS_NT;
            key[k] = 0;
            if (f < nf)
                key[k] = lh_stats_key(fr + f, channels, mode_gr);
        }
#pragma unroll
        for (int k = 0; k < LH_STATS_AHEAD; k++)
            if (f0 + k * LH_STATS_NT < nf)
                lh_stats_add(&bins, key[k], channels);
    }
    __syncthreads();
    int    *const dst = &carry[s].mode[0][0];
    for (int i = tid; i < LH_STATS_WORDS; i += LH_STATS_NT)
        dst[i] += lds[i];
}

#ifndef LH_EMU
/* The statistics launch behind an encode launch on `stream'.  Returns a hipError_t. */
extern "C" int
lh_launch_stats(const LhStreamDesc * descs, const LhFrameOut * out, int nstreams, int channels, int mode_gr, LhStatCarry * carry, void *stream)
{
    if (nstreams <= 0)
        return 0;
    if (channels < 1 || channels > 2 || mode_gr < 1 || mode_gr > 2 || !descs || !out || !carry)
        return (int) hipErrorInvalidValue;
    hipLaunchKernelGGL(lh_stats_resume_kernel, dim3((unsigned) nstreams), dim3(LH_STATS_NT), 0, (hipStream_t) stream, descs, out, nstreams,
                       channels, mode_gr, carry);
    return (int) hipGetLastError();
}
#else
/* TEST ENTRY POINTS (tests/hipemu_stats): the kernel under the fiber emulator.  Per stream: where its records start in
 * `out' (out_index) and how many the launch has (nframes); frame_begin is set off 0, as in a later round.  carry: nstreams
 * records the caller keeps from launch to launch */
extern "C" int
lh_emu_stats(const LhFrameOut * out, int nstreams, const long long *out_index, const int *nframes, int channels, int mode_gr,
             LhStatCarry * carry)
{
    std::vector < LhStreamDesc > descs((size_t) (nstreams > 0 ? nstreams : 1));
    for (int s = 0; s < nstreams; s++) {
        memset(&descs[(size_t) s], 0, sizeof(LhStreamDesc));
        descs[(size_t) s].out_index = out_index[s];
        descs[(size_t) s].frame_begin = 5;
        descs[(size_t) s].frame_end = 5 + nframes[s];
        descs[(size_t) s].mid_rel = 3;  /* (a launch in windows: the records' place does not depend on it) */
    }
    const LhStreamDesc *const d = descs.data();
    hipemu_dim3 grid = { (unsigned) nstreams, 1, 1 }, block = { LH_STATS_NT, 1, 1 };
    if (nstreams <= 0)
        return 0;
    hipemu_run(grid, block,[=] () {
               lh_stats_resume_kernel(d, out, nstreams, channels, mode_gr, carry);
               }
    );
    return 0;
}

/* the host text of lh_stats.h over n records, as this library compiled it */
extern "C" void
lh_emu_stats_host(const LhFrameOut * out, int n, int channels, int mode_gr, int *words)
{
    LhStatCarry *const c = (LhStatCarry *) words;
    /* (LH_STATS_ADD is the LDS add here, which the emulator runs as a plain one) */
    for (int f = 0; f < n; f++)
        lh_stats_count_frame(c, out + f, channels, mode_gr);
}

extern "C" int
lh_emu_stats_nt(void)
{
    return LH_STATS_NT;
}

extern "C" int
lh_emu_stats_sizeof(int which)
{
    return which == 0 ? (int) sizeof(LhStatCarry) : which == 1 ? (int) sizeof(LhFrameOut) : -1;
}
#endif
