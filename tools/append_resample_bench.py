#!/usr/bin/env python3
"""What converting the sample rate round by round costs (lamehip_batch_set_incremental_resampling): the tile kernel of
every round against the whole-stream conversion of the same samples, and a round that converts against a round that is fed
audio at the encoder's own rate.

Default workload: one GPU, 256 streams x 30 s, float32 at +/- 1.0 from a device tensor, 48 -> 44.1 kHz, CBR 128, fed in
rounds of one second.  One process; torch holds the producer's tensors.

(a) The incremental batch: per round Batch.append_ms() of Batch.append_device -- one launch of lh_append_kernel, the chunks
    as they are into the input pool --, Batch.resample_ms() of the round's encode_available -- one launch of
    lh_resample_tiles_kernel (csrc/lh_resample_dev.hip) over the tiles the appends planned -- and the wall time of append
    plus encode_available.  Medians over the rounds, the first (allocations, nothing to encode yet) and a last partial one
    left out; the sum of the tile-kernel times over ALL rounds and the finish.
(b) The whole-stream conversion of the same samples: Batch.resample_ms() of a set_input (device tensors) + encode batch
    with device resampling, lh_resample_kernel, which an incremental batch does not touch -- and (a)'s sum over it.
(c) The same rounds on a batch without conversion, fed the same tensors' first 44100 samples of every round as audio at
    44.1 kHz (tools/append_bench.py's device route; the figure of profiles/append_bench.json is quoted beside it when
    that file is there) -- and (a)'s wall time over it.

Nothing is asserted about a time.  Writes one JSON document (default profiles/append_resample_bench.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import helpers  # noqa: E402
import lamehip  # noqa: E402
from ingest_bench import spread, typed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--round-seconds", type=float, default=1.0)
    ap.add_argument("--rate-in", type=int, default=48000)
    ap.add_argument("--rate-out", type=int, default=44100)
    ap.add_argument("--brate", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_resample_bench.json"))
    a = ap.parse_args()

    torch.zeros(1, device="cuda:0")                             # torch takes the device first
    B, n, T = a.streams, int(a.rate_in * a.seconds), int(a.rate_in * a.round_seconds)
    T_out = int(a.rate_out * a.round_seconds)
    stype = lamehip.PCM_F32_UNIT
    xs = [typed(stype, helpers.synth_stream(8900 + k, n, a.rate_in)) for k in range(4)]
    # stream s: signal s % 4 rotated by 977 (s // 4) samples
    kind = np.arange(B) % len(xs)
    shift = 977 * (np.arange(B) // len(xs))
    dev_base = torch.from_numpy(np.stack(xs)).to("cuda:0")      # [4, 2, n]
    dev_kind = torch.from_numpy(kind).to("cuda:0")[:, None, None]
    dev_plane = torch.arange(2, device="cuda:0")[None, :, None]
    dev_shift = torch.from_numpy(shift).to("cuda:0")[:, None]

    def chunk_of(pos, m):
        idx = (dev_shift + pos + torch.arange(m, device="cuda:0")[None, :]) % n
        c = dev_base[dev_kind, dev_plane, idx[:, None, :]].contiguous()
        torch.cuda.synchronize()
        return c

    conv = lamehip.Encoder(a.rate_in, a.brate, out_samplerate=a.rate_out)
    same = lamehip.Encoder(a.rate_out, a.brate)
    ib = lamehip.Batch(conv, B, n)
    ib.set_device_resampling()
    ib.set_sample_type(stype)
    ib.set_incremental_resampling()
    nb = lamehip.Batch(same, B, int(a.rate_out * a.seconds) + T_out)
    nb.set_sample_type(stype)
    append, tiles, wall_conv, wall_same, frames, tiles_all = [], [], [], [], [], []
    out_conv = out_same = 0
    for rnd, pos in enumerate(range(0, n, T)):
        m = min(T, n - pos)
        chunk = chunk_of(pos, m)
        t0 = time.perf_counter()
        ib.append_device(chunk, [m] * B)
        ms = ib.append_ms()
        k = ib.encode_available()
        t1 = time.perf_counter()
        tile_ms = ib.resample_ms()
        m_out = min(T_out, m)
        t2 = time.perf_counter()
        nb.append_device(chunk, [m_out] * B)
        k2 = nb.encode_available()
        t3 = time.perf_counter()
        for s in range(B):
            out_conv += len(ib.drain(s))
            out_same += len(nb.drain(s))
        tiles_all.append(tile_ms)
        if rnd == 0 or m < T:
            continue
        append.append(ms)
        tiles.append(tile_ms)
        wall_conv.append((t1 - t0) * 1e3)
        wall_same.append((t3 - t2) * 1e3)
        frames.append(k)
        print("round %2d: append %7.3f ms   tile kernel %7.3f ms   round that converts %8.2f ms (%d frames), round at the encoder's rate "
              "%8.2f ms (%d frames)" % (rnd, ms, tile_ms, wall_conv[-1], k, wall_same[-1], k2), flush=True)
    ib.finish()
    tiles_all.append(ib.resample_ms())
    nb.finish()
    for s in range(B):
        out_conv += len(ib.drain(s))
        out_same += len(nb.drain(s))
    ib.close()
    nb.close()
    same.close()
    # (b) the whole-stream conversion of the same samples
    wb = lamehip.Batch(conv, B, n)
    wb.set_device_resampling()
    wb.set_sample_type(stype)
    whole = []
    for rep in range(3):
        for s0 in range(0, B, 32):                              # (32 streams of 30 s at a time: 0.4 GB of producer tensor)
            idx =(dev_shift[s0:s0 + 32] + torch.arange(n, device="cuda:0")[None, :]) % n
            c = dev_base[dev_kind[s0:s0 + 32], dev_plane, idx[:, None, :]].contiguous()
            torch.cuda.synchronize()
            for j in range(c.shape[0]):
                wb.set_input(s0 + j, c[j, 0], c[j, 1])
            del c
        wb.encode()
        whole.append(wb.resample_ms())
        print("whole-stream conversion, run %d: %7.3f ms (the launch's kernels %8.2f ms)" % (rep, whole[-1], wb.kernel_ms()), flush=True)
    out_whole = sum(len(wb.pack(s)) for s in range(0, B, 37))
    wb.close()
    conv.close()
    committed = None
    try:
        with open(os.path.join(ROOT, "profiles", "append_bench.json")) as f:
            committed = json.load(f)["round"]["from_device_tensor_ms"]["median"]
    except (OSError, KeyError, ValueError):
        pass
    tile_sum, whole_ms = sum(tiles_all), statistics.median(whole[1:])
    doc = dict(workload=dict(rate_in=a.rate_in, rate_out=a.rate_out, brate=a.brate, streams=B, seconds=a.seconds,
                             round_seconds=a.round_seconds, rounds_measured=len(append),
                             input="float32 at +/- 1.0, [streams, 2, samples of a round] on the device; first round left out"),
               round=dict(append_ms=spread(append), tile_kernel_ms=spread(tiles), frames_per_round=spread(frames),
                          wall_ms=spread(wall_conv), tile_kernel_share_of_wall=round(statistics.median(tiles) / statistics.median(wall_conv), 4),
                          what="per round: the append launch, the tile-kernel launch, wall time of append_device + encode_available"),
               conversion=dict(tile_kernel_ms_sum_all_rounds_and_finish=round(tile_sum, 4), launches=len(tiles_all),
                               whole_stream_ms=spread(whole[1:]), whole_stream_first_run_ms=round(whole[0], 4),
                               tiles_over_whole_stream=round(tile_sum / whole_ms, 3),
                               what="lamehip_batch_last_resample_ms: summed over the incremental batch's rounds, against one "
                                    "set_input (device) + encode of the same samples (lh_resample_kernel, unchanged)"),
               against_no_conversion=dict(same_rate_round_wall_ms=spread(wall_same),
                                          converting_over_same_rate=round(statistics.median(wall_conv) / statistics.median(wall_same), 3),
                                          append_bench_from_device_tensor_ms_median=committed,
                                          what="the same rounds on a batch at the encoder's own rate, one second of 44.1 kHz audio per "
                                               "round from the same tensors; beside it the committed figure of profiles/append_bench.json"),
               bytes_out=dict(converting=out_conv, same_rate=out_same, whole_stream_sample_of_streams=out_whole))
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
