#!/usr/bin/env python3
"""Rate conversion of a batch on the host against on the device (lamehip_batch_set_device_resampling).

Default workload: 48 kHz -> 44.1 kHz, CBR 128, 256 streams x 30 s of s16 through the pinned mirror.  One process; after
a warm-up round of each kind at the same shape the rounds alternate switch off, on, off, on.  A round's wall time runs
from its first set_pcm to the return of lamehip_batch_sync (host clock around work that ends in a synchronise); with
the switch on the conversion's own HIP-event time (resample_ms) and the launch's kernel times are recorded too, and the
conversion's traffic computed from the shapes (s16 read + float written) over resample_ms as GB/s and as a share of the
HBM peak.  The bytes of 8 streams are compared between the two paths.

Conditions: (a) in both alternations the switch-on round is faster than the switch-off round; (b) resample_ms is below
the same launch's encode-kernel time.  Writes one JSON document (default profiles/resample_bench.json) and prints it;
the exit status says whether both conditions held."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import lamehip  # noqa: E402

HBM_PEAK_GBS = 8000.0           # MI355X HBM3E, 8 TB/s


def streams(nstreams, n, rate_in):
    """nstreams distinct streams from 8 synthesised ones, each rotated by its own offset"""
    base = [helpers.synth_stream(8800 + k, n, rate_in) for k in range(8)]
    return [np.ascontiguousarray(np.roll(base[s % 8], 977 * (s // 8), axis=1)) for s in range(nstreams)]


def one_round(b, pcms):
    t0 = time.perf_counter()
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode(sync=False)
    b.sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate-in", type=int, default=48000)
    ap.add_argument("--rate-out", type=int, default=44100)
    ap.add_argument("--brate", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()

    n = int(a.rate_in * a.seconds)
    pcms = streams(a.streams, n, a.rate_in)
    enc = lamehip.Encoder(a.rate_in, a.brate, out_samplerate=a.rate_out)
    assert enc.config().samplerate == a.rate_out

    def batch(on):
        b = lamehip.Batch(enc, a.streams, n)
        b.set_device_packing()
        if on:
            b.set_device_resampling()
            b.pcm_host()        # the pinned mirror, made outside the timed rounds
        return b

    off, on = batch(False), batch(True)
    rounds = []

    def run(b, kind, note):
        wall = one_round(b, pcms)
        split, parts = b.kernel_parts_ms()
        r = dict(round=note, switch=kind, wall_ms=round(wall, 2), kernel_ms=round(b.kernel_ms(), 3),
                 kernel_parts_ms=[round(v, 3) for v in parts], resample_ms=round(b.resample_ms(), 3))
        print("%-10s %-4s wall %10.1f ms   kernels %8.2f ms (encode kernel %8.2f)   conversion %7.3f ms"
              % (note, kind, wall, r["kernel_ms"], parts[2], r["resample_ms"]), flush=True)
        return r

    run(off, "off", "warm-up")
    run(on, "on", "warm-up")
    for k in range(2):
        rounds.append(run(off, "off", "round %d" % (k + 1)))
        rounds.append(run(on, "on", "round %d" % (k + 1)))
    same = all(off.get_bytes(s) == on.get_bytes(s) and len(on.get_bytes(s)) > 0 for s in range(min(8, a.streams)))
    conv_len = on.converted(0).shape[1] * a.streams             # (equal lengths)
    off.close()
    on.close()
    enc.close()

    ons = [r for r in rounds if r["switch"] == "on"]
    offs = [r for r in rounds if r["switch"] == "off"]
    traffic = a.streams * n * 2 * 2 + conv_len * 2 * 4          # s16 read + float written, both planes
    best = min(r["resample_ms"] for r in ons)
    cond_a = all(o["wall_ms"] < f["wall_ms"] for o, f in zip(ons, offs))
    cond_b = all(0 < r["resample_ms"] < r["kernel_parts_ms"][2] for r in ons)
    doc = dict(workload=dict(rate_in=a.rate_in, rate_out=a.rate_out, brate=a.brate, streams=a.streams, seconds=a.seconds,
                             input="s16 through the pinned mirror"),
               rounds=rounds,
               conversion=dict(bytes=traffic, resample_ms=best, gb_per_s=round(traffic / best / 1e6, 1),
                               share_of_hbm_peak=round(traffic / best / 1e6 / HBM_PEAK_GBS, 4), hbm_peak_gb_per_s=HBM_PEAK_GBS),
               host_over_device_wall=round(min(f["wall_ms"] for f in offs) / min(o["wall_ms"] for o in ons), 2),
               same_bytes_8_streams=same,
               condition_a_on_faster_than_off=cond_a, condition_b_conversion_below_encode_kernel=cond_b)
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0 if (cond_a and cond_b and same) else 1


if __name__ == "__main__":
    sys.exit(main())
