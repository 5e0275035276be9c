/*
 * lh_slots.hip -- the slots of an incremental batch (gfx950): lamehip_batch_restart_stream gives a slot whose stream has
 * ended to the next stream, and everything the slot keeps in HBM from round to round starts over -- its LhStreamState from
 * the batch's initial image, its drain carry (lh_drain.hip: the header walk), its LhTagCarry (lh_tag.hip) and its
 * LhGainCarry (lh_gain.hip) zeroed -- while the records of its neighbours, which are in the middle of their streams, stay
 * as they are.
 *   lh_slot_restart_kernel  a workgroup per listed stream, ONE launch for every slot restarted in the gap between two
 *      rounds (256 slots turning over at once would otherwise be a thousand small copies of the runtime's in front of a
 *      round whose device time is some 10 ms).  A record is moved 16 bytes per lane and step; records lie back to back in
 *      their arrays, so one whose size is no multiple of 16 starts and ends off a boundary: the bytes in front of the first
 *      boundary and behind the last one go one by one.  Nothing outside the listed streams' records is written, not by a
 *      rounded-up tail either.  A record the batch does not have is a null pointer.
 * Plain loads and stores; bandwidth-bound and tiny (a slot's records are some 30 KB).
 */
#include <stdint.h>

#ifdef LH_EMU
#include "hipemu.h"
#define LH_SL_FN static inline
#else
#include <hip/hip_runtime.h>
#define LH_SL_FN static __device__ __forceinline__
#endif
#include "lh_device.h"
#include "lh_gain.h"
#include "lh_tag.h"

#define LH_SL_NT 256            /* lanes of a workgroup */

typedef uint32_t lh_sl_v4 __attribute__((vector_size(16)));

/* the `bytes' bytes at dst become those at src, or zero when src is null: the workgroup's lanes side by side.  dst and src
 * lie equally far behind a 16-byte boundary (the same record of two arrays that both start on one); where they do not,
 * everything goes byte by byte. */
LH_SL_FN void
slot_record(unsigned char *dst, const unsigned char *src, long long bytes)
{
    long long const tid = (long long) threadIdx.x;
    long long head = (long long) ((0 - (uintptr_t) dst) & 15u);
    if (head > bytes || (src && (((uintptr_t) src ^ (uintptr_t) dst) & 15u) != 0))
        head = bytes;
    long long const body = (bytes - head) / 16;
    for (long long i = tid; i < head; i += LH_SL_NT)
        dst[i] = src ? src[i] : (unsigned char) 0;
    for (long long k = tid; k < body; k += LH_SL_NT) {
        lh_sl_v4 v = { 0u, 0u, 0u, 0u };
        if (src)
            v = *(const lh_sl_v4 *) __builtin_assume_aligned(src + head + 16 * k, 16);
        *(lh_sl_v4 *) __builtin_assume_aligned(dst + head + 16 * k, 16) = v;
    }
    for (long long i = head + 16 * body + tid; i < bytes; i += LH_SL_NT)
        dst[i] = src ? src[i] : (unsigned char) 0;
}

/* grid: a workgroup per entry of `list' (stream indices in [0, nstreams); any other value is skipped).  states / states0:
 * the batch's records and their initial image; drain_carry, tag_carry, gain_carry: a record per stream, or null */
__global__ void
__launch_bounds__(LH_SL_NT)
lh_slot_restart_kernel(const int *list, int nlist, int nstreams, LhStreamState * states, const LhStreamState * states0,
                       long long *drain_carry, LhTagCarry * tag_carry, LhGainCarry * gain_carry)
{
    if ((int) blockIdx.x >= nlist)
        return;
    int const s = list[blockIdx.x];
    if (s < 0 || s >= nstreams)
        return;
    if (states && states0)
        slot_record((unsigned char *) (states + s), (const unsigned char *) (states0 + s), (long long) sizeof(LhStreamState));
    if (drain_carry)
        slot_record((unsigned char *) (drain_carry + s), nullptr, (long long) sizeof(long long));
    if (tag_carry)
        slot_record((unsigned char *) (tag_carry + s), nullptr, (long long) sizeof(LhTagCarry));
    if (gain_carry)
        slot_record((unsigned char *) (gain_carry + s), nullptr, (long long) sizeof(LhGainCarry));
}

#ifndef LH_EMU
/* The restart launch of a gap on `stream'.  Returns a hipError_t. */
extern "C" int
lh_launch_slot_restart(const int *list, int nlist, int nstreams, LhStreamState * states, const LhStreamState * states0,
                       long long *drain_carry, LhTagCarry * tag_carry, LhGainCarry * gain_carry, void *stream)
{
    if (nlist <= 0 || nstreams <= 0)
        return 0;
    hipLaunchKernelGGL(lh_slot_restart_kernel, dim3((unsigned) nlist), dim3(LH_SL_NT), 0, (hipStream_t) stream, list, nlist, nstreams, states,
                       states0, drain_carry, tag_carry, gain_carry);
    return (int) hipGetLastError();
}
#else
/* TEST ENTRY POINTS (tests/hipemu_slots): the kernel under the fiber emulator, and the sizes of its records as this
 * library compiled them */
extern "C" int
lh_emu_slot_restart(const int *list, int nlist, int nstreams, void *states, const void *states0, long long *drain_carry, void *tag_carry,
                    void *gain_carry)
{
    hipemu_dim3 grid = { (unsigned) nlist, 1, 1 }, block = { LH_SL_NT, 1, 1 };
    LhStreamState *const st = (LhStreamState *) states;
    const LhStreamState *const st0 = (const LhStreamState *) states0;
    LhTagCarry *const tg = (LhTagCarry *) tag_carry;
    LhGainCarry *const gn = (LhGainCarry *) gain_carry;
    if (nlist <= 0 || nstreams <= 0)
        return 0;
    hipemu_run(grid, block,[=] () {
               lh_slot_restart_kernel(list, nlist, nstreams, st, st0, drain_carry, tg, gn);
               }
    );
    return 0;
}

/* which: 0 LhStreamState, 1 the drain carry, 2 LhTagCarry, 3 LhGainCarry */
extern "C" int
lh_emu_slot_sizeof(int which)
{
    switch (which) {
    case 0:
        return (int) sizeof(LhStreamState);
    case 1:
        return (int) sizeof(long long);
    case 2:
        return (int) sizeof(LhTagCarry);
    case 3:
        return (int) sizeof(LhGainCarry);
    default:
        return -1;
    }
}
#endif
