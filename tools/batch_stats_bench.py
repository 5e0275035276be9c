#!/usr/bin/env python3
"""What a batch's statistics cost (lamehip_batch_set_statistics; csrc/lh_stats.hip: lh_stats_resume_kernel).

One process on one GPU, bench.py's synthetic signal at 44.1 kHz, HIP-event times; a warm-up launch, then five, median /
min / max of every figure.  Nothing is asserted about a time; the counts are compared wherever two routes give them.

  one-shot: 1024 streams x 60 s and 256 x 30 s, at CBR 128 and at -V2, on the device packer: Batch.stats_ms(), the one
      launch of the statistics kernel, next to the same launch's encode kernel (kernel_parts_ms) and all of kernel_ms();
      the bytes the kernel must touch, from the record layout -- the distinct 128-byte lines of a frame's five places
      (the record's tail, block_type / mixed_block_flag of four granules) x frames --, the time HBM needs for them at
      its measured copy rate, and the ratio of the launch's time to that;
  the parent commit's route to the same numbers at 256 x 30 s: lamehip_batch_get_frames for every stream (4928 bytes per
      frame over the host link) and a vectorised count of the records on the host, against the getter of the tables
      (704 bytes per stream);
  incremental: 256 x 30 s in rounds of one second from a device tensor (append_device), device packing + incremental
      packing + tagging, two batches that take turns round by round, the switch on and off: the launch's time per round
      next to the round's encode kernels, and the round's wall time either way.

Writes one JSON document (default profiles/batch_stats_bench.json) and prints it."""
import argparse
import ctypes as C
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
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import lamehip  # noqa: E402
from lamehip.types import LhFrameOut, LhGranule  # noqa: E402

HBM_COPY_TBS = 6.29             # measured float4 copy rate of an MI355X (8.0 TB/s on the data sheet)
RUNS = 5


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def lines_per_frame(channels, mode_gr):
    """distinct 128-byte lines the kernel reads of one record, averaged over the two ways a 4928-byte record can lie"""
    rec, gsz = C.sizeof(LhFrameOut), C.sizeof(LhGranule)
    places = [LhFrameOut.bitrate_index.offset, LhFrameOut.mode_ext.offset]
    for gr in range(mode_gr):
        for ch in range(channels):
            at = (2 * gr + ch) * gsz
            places += [at + LhGranule.block_type.offset, at + LhGranule.mixed_block_flag.offset]
    counts = [len({(f * rec + p) // 128 for p in places}) for f in range(2)]
    return sum(counts) / len(counts)


def host_count(frames, channels, mode_gr):
    """the two tables from a stream's records on the host, vectorised"""
    rec, gsz = C.sizeof(LhFrameOut), C.sizeof(LhGranule)
    raw = np.frombuffer(frames, np.uint8).reshape(-1, rec)
    bi = raw[:, LhFrameOut.bitrate_index.offset].astype(np.int64) & 15
    me = raw[:, LhFrameOut.mode_ext.offset].astype(np.int64) & 3
    mode, block = np.zeros((16, 5), np.int64), np.zeros((16, 6), np.int64)
    np.add.at(mode, (bi, 4), 1)
    if channels == 2:
        np.add.at(mode, (bi, me), 1)
    for gr in range(mode_gr):
        for ch in range(channels):
            at = (2 * gr + ch) * gsz
            bt = np.where(raw[:, at + LhGranule.mixed_block_flag.offset] != 0, 4, raw[:, at + LhGranule.block_type.offset] & 3)
            np.add.at(block, (bi, bt), 1)
            np.add.at(block, (bi, 5), 1)
    mode[15] += mode[:15].sum(axis=0)
    block[15] += block[:15].sum(axis=0)
    return mode.astype(np.int32), block.astype(np.int32)


def one_shot(name, kw, B, seconds, rate, pcm, compare_host):
    n = int(rate * seconds)
    enc = lamehip.Encoder(rate, **kw)
    cfg = enc.config()
    b = lamehip.Batch(enc, B, n)
    if not compare_host:
        b.set_device_packing()
    b.set_statistics()
    for s in range(B):
        b.set_pcm_device(s, pcm[s, 0].data_ptr(), pcm[s, 1].data_ptr(), n)
    st, enc_k, all_k = [], [], []
    for run in range(RUNS + 1):
        b.encode()
        if run:
            st.append(b.stats_ms())
            enc_k.append(b.kernel_parts_ms()[1][2] if b.kernel_parts_ms()[0] else b.kernel_ms())
            all_k.append(b.kernel_ms())
    frames = sum(b.frames(s) for s in range(B))
    lines = lines_per_frame(cfg.channels, cfg.mode_gr)
    nbytes = lines * 128 * frames
    hbm_ms = nbytes / (HBM_COPY_TBS * 1e12) * 1e3
    med = statistics.median
    doc = dict(settings=kw, streams=B, seconds=seconds, frames=frames, windows=b.windows(),
               stats_launch_ms=spread(st), encode_kernel_ms=spread(enc_k), all_kernels_ms=spread(all_k),
               stats_share_of_the_encode_kernel=round(med(st) / med(enc_k), 6),
               lines_of_128_bytes_per_frame=lines, bytes_the_kernel_must_touch=int(nbytes),
               record_bytes_of_the_launch=int(frames * C.sizeof(LhFrameOut)),
               hbm_ms_for_those_bytes=round(hbm_ms, 4), hbm_rate_assumed_tb_s=HBM_COPY_TBS,
               launch_over_hbm_time=round(med(st) / hbm_ms, 1) if hbm_ms > 0 else None,
               effective_gb_s=round(nbytes / (med(st) * 1e-3) / 1e9, 1))
    if compare_host:
        t0 = time.perf_counter()
        every = b.statistics_all()
        t1 = time.perf_counter()
        got = [b.get_frames(s) for s in range(B)]
        t2 = time.perf_counter()
        counted = [host_count(bytes(f), cfg.channels, cfg.mode_gr) for f in got]
        t3 = time.perf_counter()
        same = all((np.concatenate([m.ravel(), k.ravel()]) == every[s]).all() for s, (m, k) in enumerate(counted))
        doc["parent_route"] = dict(get_frames_all_streams_ms=round((t2 - t1) * 1e3, 2), host_count_ms=round((t3 - t2) * 1e3, 2),
                                   record_bytes_brought_home=int(frames * C.sizeof(LhFrameOut)),
                                   getter_of_the_tables_ms=round((t1 - t0) * 1e3, 3), table_bytes_brought_home=B * 704,
                                   counts_equal=bool(same))
    print("%s %d x %.0f s: statistics %.4f ms, encode kernel %.2f ms" % (name, B, seconds, med(st), med(enc_k)), flush=True)
    b.close()
    enc.close()
    return doc


def rounds(name, kw, B, seconds, rate, pcm):
    n, T = int(rate * seconds), rate
    enc = lamehip.Encoder(rate, **kw)
    batches = {}
    for mode in ("on", "off"):
        b = lamehip.Batch(enc, B, n)
        b.set_device_packing()
        b.set_incremental_packing()
        b.set_incremental_tagging()
        if mode == "on":
            b.set_statistics()
        batches[mode] = b
    wall, st, kern = dict(on=[], off=[]), [], []
    same = True
    for rnd, pos in enumerate(range(0, n, T)):
        m = min(T, n - pos)
        chunk = pcm[:, :, pos:pos + m]
        got = {}
        for mode in (("on", "off") if rnd % 2 else ("off", "on")):
            b = batches[mode]
            t0 = time.perf_counter()
            b.append_device(chunk, [m] * B)
            b.encode_available()
            got[mode] = [b.drain_view(s).tobytes() for s in range(B)]
            t1 = time.perf_counter()
            if rnd > 0 and m == T:
                wall[mode].append((t1 - t0) * 1e3)
        same = same and got["on"] == got["off"]
        if rnd > 0 and m == T:
            st.append(batches["on"].stats_ms())
            kern.append(batches["on"].kernel_ms())
    for b in batches.values():
        b.finish()
    frames = sum(batches["on"].frames(s) for s in range(B))
    counted = int(batches["on"].statistics_all()[:, 15 * 5 + 4].sum())
    for b in batches.values():
        b.close()
    enc.close()
    med = statistics.median
    print("%s rounds: statistics %.4f ms per round, wall on %.2f / off %.2f ms" % (name, med(st), med(wall["on"]), med(wall["off"])), flush=True)
    return dict(settings=kw, streams=B, seconds=seconds, rounds_measured=len(st), stats_launch_ms=spread(st), encode_kernels_ms=spread(kern),
                stats_share_of_the_encode_kernels=round(med(st) / med(kern), 6),
                round_wall_ms=dict(switch_on=spread(wall["on"]), switch_off=spread(wall["off"]),
                                   on_over_off=round(med(wall["on"]) / med(wall["off"]), 4)),
                drains_equal_with_the_switch_on_and_off=bool(same), frames=frames, frames_counted=counted)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--big", type=int, nargs=2, default=[1024, 60], metavar=("STREAMS", "SECONDS"))
    ap.add_argument("--small", type=int, nargs=2, default=[256, 30], metavar=("STREAMS", "SECONDS"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_stats_bench.json"))
    a = ap.parse_args()
    torch.zeros(1, device="cuda:0")                             # torch takes the device first
    dev = torch.device("cuda:0")
    settings = (("cbr128", dict(brate=128)), ("vbr2", dict(vbr_q=2)))
    doc = dict(workload=dict(rate=a.rate, signal="bench.py's synthetic signal, int16 on the device", runs=RUNS, warmup=1,
                             times="HIP events (launches), time.perf_counter (walls)"),
               one_shot={}, incremental={})
    for label, (B, seconds) in (("big", a.big), ("small", a.small)):
        pcm = bench.synth_on_device(torch, B, int(a.rate * seconds), a.rate, 1000, dev)
        torch.cuda.synchronize()
        for name, kw in settings:
            doc["one_shot"]["%s_%dx%d" % (name, B, seconds)] = one_shot(name, kw, B, seconds, a.rate, pcm, False)
        if label == "small":
            doc["one_shot"]["cbr128_%dx%d_host_packed" % (B, seconds)] = one_shot("cbr128 (host-packed)", dict(brate=128), B, seconds,
                                                                                 a.rate, pcm, True)
            for name, kw in settings:
                doc["incremental"][name] = rounds(name, kw, B, seconds, a.rate, pcm)
        del pcm
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
