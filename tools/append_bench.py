#!/usr/bin/env python3
"""What feeding an incremental batch from the GPU costs (lamehip_batch_append_device): the append kernel against the
runtime's own copy, and a round fed from a device tensor against the same round fed as s16 from host memory.

Default workload: 44.1 kHz, CBR 128, 256 streams x 30 s, fed in rounds of one second.  One process; torch holds the
producer's tensors.  Per round:

(a) Batch.append_ms() of Batch.append_device for a float32 unit-scale tensor [B, 2, T] on the device -- one launch of
    lh_append_kernel (csrc/lh_ingest.hip) -- and, alternating with it, a hipMemcpyAsync device-to-device of the bytes the
    kernel reads (it writes as many: the same traffic), timed with HIP events on a stream of its own; the bandwidth the
    kernel's read + written bytes amount to.
(b) wall time of the round, append plus encode_available, through append_device -- against the same samples rounded to
    int16 in host memory through lamehip_batch_append (one call per stream, the pinned arena, one copy, the scatter kernel)
    plus encode_available on a second batch: the only route there was before the typed appends.

The first round (allocations, nothing to encode yet) is left out; median, min and max over the others.  Nothing is asserted
about a time.  Writes one JSON document (default profiles/append_bench.json) and prints it."""
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
from ingest_bench import HBM_PEAK_GBS, DeviceCopy, rounded, spread, typed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--round-seconds", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--brate", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_bench.json"))
    a = ap.parse_args()

    torch.zeros(1, device="cuda:0")                             # torch takes the device first
    B, n, T = a.streams, int(a.rate * a.seconds), int(a.rate * a.round_seconds)
    stype = lamehip.PCM_F32_UNIT
    base = [helpers.synth_stream(8800 + k, n, a.rate) for k in range(4)]
    xs = [typed(stype, b) for b in base]
    rs = [rounded(stype, x) for x in xs]
    # stream s: signal s % 4 rotated by 977 (s // 4) samples
    kind = np.arange(B) % len(xs)
    shift = 977 * (np.arange(B) // len(xs))
    dev_base = torch.from_numpy(np.stack(xs)).to("cuda:0")      # [4, 2, n]
    dev_kind = torch.from_numpy(kind).to("cuda:0")[:, None, None]
    dev_plane = torch.arange(2, device="cuda:0")[None, :, None]
    dev_shift = torch.from_numpy(shift).to("cuda:0")[:, None]
    lib = lamehip.load_library()
    enc = lamehip.Encoder(a.rate, a.brate)
    tb = lamehip.Batch(enc, B, n)
    tb.set_sample_type(stype)
    sb = lamehip.Batch(enc, B, n)
    read_bytes = B * 2 * T * 4
    copy = DeviceCopy(lib, read_bytes)
    append, copies, wall_dev, wall_host, frames = [], [], [], [], []
    out_dev = out_host = 0
    for rnd, pos in enumerate(range(0, n, T)):
        m = min(T, n - pos)
        # the producer's chunk of this round, [B, 2, m] on the device, and the same samples as shorts on the host
        idx = (dev_shift + pos + torch.arange(m, device="cuda:0")[None, :]) % n
        chunk = dev_base[dev_kind, dev_plane, idx[:, None, :]].contiguous()
        torch.cuda.synchronize()
        hidx = [(int(shift[s]) + pos + np.arange(m)) % n for s in range(B)]
        hl = [np.ascontiguousarray(rs[kind[s]][0][hidx[s]]) for s in range(B)]
        hr = [np.ascontiguousarray(rs[kind[s]][1][hidx[s]]) for s in range(B)]
        t0 = time.perf_counter()
        tb.append_device(chunk, [m] * B)
        ms = tb.append_ms()
        k = tb.encode_available()
        t1 = time.perf_counter()
        c = copy.run(B * 2 * m * 4)
        t2 = time.perf_counter()
        for s in range(B):
            sb.append(s, hl[s], hr[s])
        k2 = sb.encode_available()
        t3 = time.perf_counter()
        assert k == k2
        for s in range(B):
            out_dev += len(tb.drain(s))
            out_host += len(sb.drain(s))
        if rnd == 0 or m < T:
            continue
        append.append(ms)
        copies.append(c)
        wall_dev.append((t1 - t0) * 1e3)
        wall_host.append((t3 - t2) * 1e3)
        frames.append(k)
        print("round %2d: append %7.3f ms   copy of the bytes read %7.3f ms   round from the device %8.2f ms, as s16 from the host %8.2f ms"
              "   (%d frames)" % (rnd, ms, c, wall_dev[-1], wall_host[-1], k), flush=True)
    tb.finish()
    sb.finish()
    for s in range(B):
        out_dev += len(tb.drain(s))
        out_host += len(sb.drain(s))
    copy.close()
    tb.close()
    sb.close()
    enc.close()
    med = statistics.median(append)
    doc = dict(workload=dict(rate=a.rate, brate=a.brate, streams=B, seconds=a.seconds, round_seconds=a.round_seconds, rounds_measured=len(append),
                             input="float32 at +/- 1.0, [streams, 2, samples of a round] on the device; first round left out"),
               hbm_peak_gb_per_s=HBM_PEAK_GBS,
               append=dict(append_ms=spread(append), bytes_read=read_bytes, bytes_written=read_bytes,
                           append_gb_per_s=round(2 * read_bytes / med / 1e6, 1),
                           append_share_of_hbm_peak=round(2 * read_bytes / med / 1e6 / HBM_PEAK_GBS, 4),
                           copy_of_read_bytes_ms=spread(copies), append_over_copy_of_read_bytes=round(med / statistics.median(copies), 3)),
               round=dict(frames_per_round=spread(frames), from_device_tensor_ms=spread(wall_dev), as_s16_from_host_ms=spread(wall_host),
                          host_over_device=round(statistics.median(wall_host) / statistics.median(wall_dev), 3),
                          what="wall time of append + encode_available; the host route: lamehip_batch_append per stream on an s16 batch, "
                               "the shorts already rounded"),
               bytes_out=dict(from_device_tensor=out_dev, as_s16_from_host=out_host))
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
