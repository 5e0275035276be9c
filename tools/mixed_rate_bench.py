#!/usr/bin/env python3
"""What one launch for all input rates costs (lamehip_batch_set_stream_in_samplerate; csrc/lh_resample_dev.hip:
lh_resample_mixed_tiles_kernel) against what a user had to do before it existed: one batch per input rate.

Workload: one GPU, 256 streams x 30 s of float32 at +/- 1.0 from a device tensor, in rounds of one second; four classes of
64 streams each -- 48, 32 and 22.05 kHz, and 44.1 kHz, which passes through -- all to 44.1 kHz CBR 128.

(a) this build, ONE batch of 256 slots at the four rates: per round Batch.resample_ms() of encode_available -- the mixed
    launch -- and the wall time of append_device + encode_available; the median over the rounds (the first left out), five
    repeats.
(b) the PARENT build (--parent-lib, loaded through LAMEHIP_LIB as tools/ab.sh alternates builds), FOUR batches of 64 slots:
    three single-rate converting batches' resample_ms() and a plain 44.1 kHz batch's append_ms() (there the append kernel
    does what the pass-through tiles do) on the same streams and chunks, summed per round; median, five repeats, and their
    spread -- the bar (a) is held against.
(c) switch off: a single-rate converting batch of 256 slots at 48 kHz on this build and on the parent's, the two libraries
    alternating: resample_ms() and round wall time (profiles/mixed_rate_ab.json).

Every measurement runs in a child process of this script (a library is chosen when a process starts); the parent process
never opens the GPU, one child runs at a time.  Nothing is asserted about a time.  Writes profiles/mixed_rate_bench.json
and profiles/mixed_rate_ab.json and prints them."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = 44100
CLASSES = [48000, 32000, 22050, 44100]


def spread(v):
    v = [float(x) for x in v]
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def child(a):
    """one role in this process: prints one JSON line"""
    import torch
    torch.zeros(1, device="cuda:0")                             # torch takes the device first
    sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
    import lamehip
    stype = lamehip.PCM_F32_UNIT
    rounds = int(a.seconds)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(9100)
    chunk_all = (torch.rand((a.streams, 2, max(CLASSES)), device="cuda:0", generator=gen) - 0.5) * 1.6
    torch.cuda.synchronize()
    per = a.streams // len(CLASSES)

    def converting(rate, first, n):
        enc = lamehip.Encoder(rate, a.brate, out_samplerate=OUT)
        b = lamehip.Batch(enc, n, rate * rounds)
        b.set_device_resampling()
        b.set_sample_type(stype)
        b.set_incremental_resampling()
        return enc, b, chunk_all[first:first + n, :, :rate], [rate] * n

    def run(batches, figure):
        """`rounds' rounds over the batches (enc, batch, chunk, lengths): per round the sum of figure(batch) and the wall time"""
        ms, wall = [], []
        for rnd in range(rounds):
            t0 = time.perf_counter()
            tot = 0.0
            for enc, b, chunk, lengths in batches:
                b.append_device(chunk, lengths)
                b.encode_available()
                tot += figure(enc, b)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(tot)
            for enc, b, chunk, lengths in batches:
                for s in range(b.n):
                    b.drain(s)
        for enc, b, chunk, lengths in batches:
            b.finish()
            b.close()
            enc.close()
        return statistics.median(ms[1:]), statistics.median(wall[1:])

    res = []
    for rep in range(a.repeats):
        if a.role == "mixed":
            enc, b, chunk, _ = converting(CLASSES[0], 0, a.streams)
            lengths = []
            for s in range(a.streams):
                hz = CLASSES[min(s // per, len(CLASSES) - 1)]
                b.set_stream_in_samplerate(s, hz)
                lengths.append(hz)
            res.append(run([(enc, b, chunk_all, lengths)], lambda e, x: x.resample_ms()))
        elif a.role == "today":
            batches = [converting(hz, k * per, per) for k, hz in enumerate(CLASSES[:3])]
            enc = lamehip.Encoder(OUT, a.brate)
            pb = lamehip.Batch(enc, per, OUT * rounds)
            pb.set_sample_type(stype)
            batches.append((enc, pb, chunk_all[3 * per:4 * per, :, :OUT], [OUT] * per))
            res.append(run(batches, lambda e, x: x.resample_ms() if x is not pb else x.append_ms()))
        else:                                                   # "single": one converting batch of all slots at 48 kHz
            res.append(run([converting(CLASSES[0], 0, a.streams)], lambda e, x: x.resample_ms()))
    print(json.dumps(dict(role=a.role, lib=os.environ.get("LAMEHIP_LIB", ""), ms=[r[0] for r in res], wall_ms=[r[1] for r in res])), flush=True)
    return 0


def spawn(a, role, lib, repeats):
    env = dict(os.environ)
    env.pop("LAMEHIP_LIB", None)
    if lib:
        env["LAMEHIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--repeats", str(repeats), "--streams", str(a.streams),
           "--seconds", str(a.seconds), "--brate", str(a.brate)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise RuntimeError("%s (%s) failed:\n%s" % (role, lib or "this build", r.stdout[-3000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="liblamehip.so of the parent commit (tools/ab.sh's second build)")
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--brate", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=500)
    ap.add_argument("--role", choices=["mixed", "today", "single"], help="(internal: a child process's measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_rate_bench.json"))
    ap.add_argument("--out-ab", default=os.path.join(ROOT, "profiles", "mixed_rate_ab.json"))
    a = ap.parse_args()
    if a.role:
        return child(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's liblamehip.so")
    mixed = spawn(a, "mixed", None, a.repeats)
    print("this build, one batch at four rates: resample_ms %r" % mixed["ms"], flush=True)
    today = spawn(a, "today", a.parent_lib, a.repeats)
    print("parent build, four batches: resample_ms + append_ms %r" % today["ms"], flush=True)
    m, t = statistics.median(mixed["ms"]), statistics.median(today["ms"])
    t_spread = max(today["ms"]) - min(today["ms"])
    doc = dict(workload=dict(streams=a.streams, seconds=a.seconds, round_seconds=1.0, classes_hz=CLASSES, rate_out=OUT, brate=a.brate,
                             input="float32 at +/- 1.0, [streams, 2, samples of a round] on the device; first round left out",
                             repeats=a.repeats),
               mixed_one_launch=dict(resample_ms=spread(mixed["ms"]), round_wall_ms=spread(mixed["wall_ms"]), runs=mixed["ms"],
                                     what="this build: one batch, every slot at its own rate; per round Batch.resample_ms()"),
               parent_four_batches=dict(sum_ms=spread(today["ms"]), round_wall_ms=spread(today["wall_ms"]), runs=today["ms"],
                                        spread_ms=round(t_spread, 4),
                                        what="the parent's library: three single-rate batches' resample_ms + a plain batch's append_ms"),
               bar=dict(mixed_over_sum=round(m / t, 3), difference_ms=round(m - t, 4), parent_spread_ms=round(t_spread, 4),
                        met=bool(m <= t + t_spread),
                        what="the mixed launch takes no longer than the sum, beyond the spread of the parent's own repeated runs"))
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ab = dict(this=dict(ms=[], wall_ms=[]), parent=dict(ms=[], wall_ms=[]))
    for k in range(a.ab_rounds):
        for who, lib in (("parent", a.parent_lib), ("this", None)):
            r = spawn(a, "single", lib, 1)
            ab[who]["ms"] += r["ms"]
            ab[who]["wall_ms"] += r["wall_ms"]
            print("switch off, %s build: resample_ms %.4f, round %.2f ms" % (who, r["ms"][0], r["wall_ms"][0]), flush=True)
    doc = dict(workload=dict(streams=a.streams, seconds=a.seconds, rate_in=CLASSES[0], rate_out=OUT, brate=a.brate,
                             what="a single-rate incremental converting batch that never calls lamehip_batch_set_stream_in_samplerate; "
                                  "the two libraries alternate, one process each"),
               resample_ms=dict(this=spread(ab["this"]["ms"]), parent=spread(ab["parent"]["ms"])),
               round_wall_ms=dict(this=spread(ab["this"]["wall_ms"]), parent=spread(ab["parent"]["wall_ms"])),
               runs=ab)
    text = json.dumps(doc, indent=1)
    print(text)
    with open(a.out_ab, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
