#!/usr/bin/env python3
"""What ending and restarting single streams buys a service whose streams come and go (lamehip_batch_end_stream /
_restart_stream), and what the restart launch costs.

Workload: 44.1 kHz, CBR 128, 256 slots, utterances of seeded random lengths between 2 and 10 s cut from a device tensor
(float32 at +/- 1.0), rounds of one second through lamehip_batch_append_device, on the full device-resident configuration:
device packing, incremental packing, incremental tagging.  The same utterances go through two loops:

  slots     a pool of 256 slots.  A slot whose utterance is through ends with the round (end_stream), its last bytes and its
            tag frame are taken right behind that round, and it takes the next utterance in the gap (restart_stream).
  baseline  the only way the API allowed before: generations of 256 utterances that wait for their longest member --
            encode_available round by round, then finish, all drains and tags, reset.

Reported for both: audio seconds finished per wall second, the mean slot occupancy (slots that were given samples in a round,
over all rounds), the mean time from a stream's last sample -- the start of the round that hands it over -- to its finished
file (last bytes and tag in host memory) -- the loops run as fast as the device allows, so these are milliseconds; for a live
producer the figure is the ROUNDS a finished utterance waits for its file behind the round that took its last sample (at one
round a second: seconds), 0 in the slots loop by construction --; for the slots loop the restart launch's time per round
(Batch.restart_ms(), rounds that had one) and its share of the round's device time (append + encode + drain + tag + restart
launches).  Every utterance's file is hashed in both loops and the hashes compared; nothing is asserted about a time.
Writes one JSON document (default profiles/slots_bench.json) and prints it."""
import argparse
import hashlib
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


def full_batch(enc, B, cap):
    b = lamehip.Batch(enc, B, cap)
    b.set_sample_type(lamehip.PCM_F32_UNIT)
    b.set_device_packing()
    b.set_incremental_packing()
    b.set_incremental_tagging()
    return b


class Feed:
    """the round's [B, 2, T] tensor: slot s's next samples of its utterance (kind, shift, position), gathered on the device"""

    def __init__(self, base, B, T):
        self.base, self.B, self.T, self.n = base, B, T, base.shape[2]
        self.plane = torch.arange(2, device="cuda:0")[None, :, None]
        self.ramp = torch.arange(T, device="cuda:0")[None, :]

    def chunk(self, kind, start):
        k = torch.from_numpy(np.asarray(kind, dtype=np.int64)).to("cuda:0")[:, None, None]
        at = torch.from_numpy(np.asarray(start, dtype=np.int64)).to("cuda:0")[:, None]
        idx = (at + self.ramp) % self.n
        x = self.base[k, self.plane, idx[:, None, :]].contiguous()
        torch.cuda.synchronize()                                # the producer has finished
        return x


def slots_loop(enc, feed, B, T, cap, lens, kinds, shifts):
    b = full_batch(enc, B, cap)
    N = len(lens)
    queue = list(range(N))
    cur = [queue.pop(0) if queue else None for _ in range(B)]
    pos = [0] * B
    sha = [hashlib.sha1() for _ in range(N)]
    tags = [b""] * N
    latency, occupancy, restart_ms, restart_share, device_ms, rounds = [], [], [], [], [], 0
    t_start = time.perf_counter()
    while any(c is not None for c in cur):
        ns = [0 if cur[s] is None else min(T, lens[cur[s]] - pos[s]) for s in range(B)]
        x = feed.chunk([0 if cur[s] is None else kinds[cur[s]] for s in range(B)],
                       [0 if cur[s] is None else shifts[cur[s]] + pos[s] for s in range(B)])
        t0 = time.perf_counter()
        b.append_device(x, ns)
        ending = []
        for s in range(B):
            pos[s] += ns[s]
            if cur[s] is not None and pos[s] == lens[cur[s]]:
                b.end_stream(s)
                ending.append(s)
        b.encode_available()
        dev = b.append_ms() + b.kernel_ms() + b.drain_ms() + b.tag_ms() + b.restart_ms()
        device_ms.append(dev)
        if b.restart_ms() > 0.0:
            restart_ms.append(b.restart_ms())
            restart_share.append(b.restart_ms() / dev)
        for s in range(B):
            if cur[s] is not None:
                sha[cur[s]].update(b.drain_view(s).tobytes())
        for s in ending:
            tags[cur[s]] = b.tag(s)
            latency.append((time.perf_counter() - t0) * 1e3)
            b.restart_stream(s)
            cur[s], pos[s] = (queue.pop(0) if queue else None), 0
        occupancy.append(sum(1 for n in ns if n > 0) / B)
        rounds += 1
    wall = time.perf_counter() - t_start
    b.close()
    return dict(wall_s=wall, rounds=rounds, latency=latency, waited=[0] * N, occupancy=occupancy, restart_ms=restart_ms, restart_share=restart_share,
                device_ms=device_ms, files=[sha[u].hexdigest() + hashlib.sha1(tags[u]).hexdigest() for u in range(N)])


def baseline_loop(enc, feed, B, T, cap, lens, kinds, shifts):
    b = full_batch(enc, B, cap)
    N = len(lens)
    sha = [hashlib.sha1() for _ in range(N)]
    tags = [b""] * N
    latency, waited, occupancy, device_ms, rounds = [], [], [], [], 0
    t_start = time.perf_counter()
    for g0 in range(0, N, B):
        members = list(range(g0, min(g0 + B, N)))
        pos = [0] * B
        handed = {}
        while any(pos[k] < lens[u] for k, u in enumerate(members)):
            ns = [min(T, lens[members[s]] - pos[s]) if s < len(members) else 0 for s in range(B)]
            x = feed.chunk([kinds[members[s]] if s < len(members) else 0 for s in range(B)],
                           [shifts[members[s]] + pos[s] if s < len(members) else 0 for s in range(B)])
            t0 = time.perf_counter()
            b.append_device(x, ns)
            for k, u in enumerate(members):
                pos[k] += ns[k]
                if ns[k] > 0 and pos[k] == lens[u]:
                    handed[u] = (t0, rounds)
            b.encode_available()
            device_ms.append(b.append_ms() + b.kernel_ms() + b.drain_ms() + b.tag_ms())
            for k, u in enumerate(members):
                sha[u].update(b.drain_view(k).tobytes())
            occupancy.append(sum(1 for n in ns if n > 0) / B)
            rounds += 1
        b.finish()
        for k, u in enumerate(members):
            sha[u].update(b.drain_view(k).tobytes())
        out, sizes = b.tags_all()
        done = time.perf_counter()
        for k, u in enumerate(members):
            tags[u] = bytes(out[k, :sizes[k]])
            latency.append((done - handed[u][0]) * 1e3)
            waited.append(rounds - 1 - handed[u][1])
        b.reset()
    wall = time.perf_counter() - t_start
    b.close()
    return dict(wall_s=wall, rounds=rounds, latency=latency, waited=waited, occupancy=occupancy, device_ms=device_ms,
                files=[sha[u].hexdigest() + hashlib.sha1(tags[u]).hexdigest() for u in range(N)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--utterances", type=int, default=2048)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--max-seconds", type=float, default=10.0)
    ap.add_argument("--round-seconds", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--seed", type=int, default=4711)
    ap.add_argument("--baseline-only", action="store_true",
                    help="the baseline loop alone, which makes none of the new calls: for a library that does not have them (LAMEHIP_LIB), "
                         "to compare what a round without them costs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slots_bench.json"))
    a = ap.parse_args()

    torch.zeros(1, device="cuda:0")                             # torch takes the device first
    B, N, T = a.slots, a.utterances, int(a.rate * a.round_seconds)
    rng = np.random.default_rng(a.seed)
    lens = [int(a.rate * rng.uniform(a.min_seconds, a.max_seconds)) for _ in range(N)]
    n = int(a.rate * a.max_seconds)
    xs = [typed(lamehip.PCM_F32_UNIT, helpers.synth_stream(8900 + k, n, a.rate)) for k in range(4)]
    kinds = [u % len(xs) for u in range(N)]
    shifts = [977 * (u // len(xs)) % n for u in range(N)]
    feed = Feed(torch.from_numpy(np.stack(xs)).to("cuda:0"), B, T)
    enc = lamehip.Encoder(a.rate, brate=128)
    cap = max(lens) + 1
    # (a short pass of each loop first: allocations, the first launches)
    warm = min(N, B + B // 2)
    loops = dict(baseline=baseline_loop) if a.baseline_only else dict(slots=slots_loop, baseline=baseline_loop)
    for loop in loops.values():
        loop(enc, feed, B, T, cap, lens[:warm], kinds, shifts)
    runs = {name: loop(enc, feed, B, T, cap, lens, kinds, shifts) for name, loop in loops.items()}
    enc.close()
    audio_s = sum(lens) / a.rate
    doc = dict(workload=dict(rate=a.rate, settings="CBR 128", slots=B, utterances=N, seconds=[a.min_seconds, a.max_seconds], seed=a.seed,
                             audio_seconds=round(audio_s, 1), round_seconds=a.round_seconds,
                             input="float32 at +/- 1.0, [slots, 2, samples of a round] gathered on the device; device packing, "
                                   "incremental packing, incremental tagging",
                             round="append_device + (end_stream) + encode_available + the drain of every fed slot (in place, copied "
                                   "out) + (tag, restart_stream)"))
    for name, r in runs.items():
        doc[name] = dict(rounds=r["rounds"], wall_s=round(r["wall_s"], 3), audio_seconds_per_wall_second=round(audio_s / r["wall_s"], 1),
                         mean_slot_occupancy=round(statistics.mean(r["occupancy"]), 4),
                         last_sample_to_finished_file_ms=dict(mean=round(statistics.mean(r["latency"]), 2), **spread(r["latency"])),
                         rounds_waited_for_the_finished_file=dict(mean=round(statistics.mean(r["waited"]), 3), max=max(r["waited"])),
                         device_ms_per_round=spread(r["device_ms"]))
    if not a.baseline_only:
        s = runs["slots"]
        doc["slots"]["restart_launch_ms_per_round"] = spread(s["restart_ms"])
        doc["slots"]["restart_share_of_the_rounds_device_time"] = spread(s["restart_share"])
        doc["slots_over_baseline"] = dict(
            audio_seconds_per_wall_second=round(runs["baseline"]["wall_s"] / s["wall_s"], 3),
            mean_last_sample_to_finished_file=round(statistics.mean(s["latency"]) / statistics.mean(runs["baseline"]["latency"]), 4))
        doc["files_equal_in_both_loops"] = bool(s["files"] == runs["baseline"]["files"])
    else:
        doc["files_sha1"] = hashlib.sha1("".join(runs["baseline"]["files"]).encode()).hexdigest()
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
