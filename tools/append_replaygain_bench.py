#!/usr/bin/env python3
"""What ReplayGain costs an incremental batch (lamehip_batch_set_incremental_replaygain): the gain launch of every round
(lh_gain_resume_kernel, csrc/lh_gain.hip) against the whole-stream gain kernel on the same samples.

Default workload, as tools/append_bench.py: 44.1 kHz, CBR 128, 256 streams x 30 s, float32 at +/- 1.0 in one device tensor
[B, 2, n], fed in rounds of one second through Batch.append_device.  One process; torch holds the producer's tensor.

(a) Two incremental batches take the same rounds, one with the switch and one without, in alternating order: per round
    Batch.gain_ms() (the round's gain launch, HIP events), Batch.append_ms() and the wall time of append_device +
    encode_available.  The first round (allocations, nothing to encode yet) is left out of the medians; the SUM of the gain
    times is over all rounds, the finish's flush round included.
(b) A whole-stream batch with set_replaygain takes the same streams from the same tensor (set_input from device slices) and
    encodes them `--reps' times, every stream declared again before each: Batch.gain_ms() of lh_gain_kernel.
(c) The floor of a launch on this machine: a 16-byte device-to-device copy between two events (`empty_launch_ms'), and the
    gain launch of a round that brings every stream ONE sample on a third incremental batch -- launch, carry restored and
    stored, one run of 64 (`one_sample_round_ms').
The document says what the rounds' sum exceeds the whole-stream time by, and what 30 empty launches plus a tenth of the
whole-stream time would allow.  Nothing is asserted about a time.  Writes one JSON document (default
profiles/append_replaygain_bench.json) and prints it."""
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
from ingest_bench import DeviceCopy, spread, typed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--round-seconds", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--brate", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-switch-batch", action="store_true", help="leave the batch with the switch out (a library without it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_replaygain_bench.json"))
    a = ap.parse_args()

    torch.zeros(1, device="cuda:0")                             # torch takes the device first
    B, n, T = a.streams, int(a.rate * a.seconds), int(a.rate * a.round_seconds)
    stype = lamehip.PCM_F32_UNIT
    xs = [typed(stype, helpers.synth_stream(8900 + k, n, a.rate)) for k in range(4)]
    # stream s: signal s % 4 rotated by 977 (s // 4) samples; all of them in one tensor [B, 2, n]
    dev_base = torch.from_numpy(np.stack(xs)).to("cuda:0")
    full = torch.empty((B, 2, n), dtype=torch.float32, device="cuda:0")
    for s in range(B):
        full[s] = torch.roll(dev_base[s % 4], -977 * (s // 4), dims=1)
    torch.cuda.synchronize()
    lib = lamehip.load_library()
    enc = lamehip.Encoder(a.rate, a.brate)

    def incremental(switch):
        b = lamehip.Batch(enc, B, n)
        b.set_sample_type(stype)
        if switch:
            b.set_incremental_replaygain()
        return b

    batches = {"off": incremental(False)}
    if not a.no_switch_batch:
        batches["on"] = incremental(True)
    per = {k: dict(gain=[], append=[], wall=[], gain_all=[]) for k in batches}
    frames, out_bytes = [], {k: 0 for k in batches}
    for rnd, pos in enumerate(range(0, n, T)):
        m = min(T, n - pos)
        chunk = full[:, :, pos:pos + m]
        ks = {}
        for name in (sorted(batches) if rnd % 2 == 0 else sorted(batches, reverse=True)):
            b = batches[name]
            t0 = time.perf_counter()
            b.append_device(chunk, [m] * B)
            ams = b.append_ms()
            ks[name] = b.encode_available()
            wall = (time.perf_counter() - t0) * 1e3
            for s in range(B):
                out_bytes[name] += len(b.drain(s))
            per[name]["gain_all"].append(b.gain_ms())
            if rnd > 0 and m == T:
                per[name]["gain"].append(b.gain_ms())
                per[name]["append"].append(ams)
                per[name]["wall"].append(wall)
        assert len(set(ks.values())) == 1
        if rnd > 0 and m == T:
            frames.append(ks["off"])
        print("round %2d: " % rnd + "   ".join("%s: gain %7.3f ms, round %8.2f ms" % (k, per[k]["gain_all"][-1], per[k]["wall"][-1] if rnd > 0 and m == T else 0.0)
                                                 for k in sorted(batches)), flush=True)
    gains = None
    for name, b in batches.items():
        b.finish()
        per[name]["gain_all"].append(b.gain_ms())
        for s in range(B):
            out_bytes[name] += len(b.drain(s))
        if name == "on":
            gains = [b.radio_gain(s) for s in range(B)]
        b.close()
    assert len(set(out_bytes.values())) == 1, out_bytes

    # (b) the whole-stream kernel on the same samples
    wb = lamehip.Batch(enc, B, n)
    wb.set_sample_type(stype)
    wb.set_replaygain()
    for s in range(B):
        wb.set_input(s, full[s, 0], full[s, 1])
    whole = []
    for rep in range(a.reps):
        for s in range(B):
            wb.set_length(s, n)
        wb.encode()
        wb.sync()
        whole.append(wb.gain_ms())
        print("whole streams, rep %d: gain %8.3f ms" % (rep, whole[-1]), flush=True)
    whole_gains = [wb.radio_gain(s) for s in range(B)]
    wb.close()

    # (c) the floor of a launch
    copy = DeviceCopy(lib, 4096)
    empty = [copy.run(16) for _ in range(12)][2:]
    copy.close()
    tiny = []
    if not a.no_switch_batch:
        tbatch = incremental(True)
        for rep in range(12):
            tbatch.append_device(full[:, :, rep:rep + 1], [1] * B)
            tbatch.encode_available()
            tiny.append(tbatch.gain_ms())
        tbatch.close()
        tiny = tiny[2:]
    enc.close()

    doc = dict(workload=dict(rate=a.rate, brate=a.brate, streams=B, seconds=a.seconds, round_seconds=a.round_seconds,
                             rounds=len(per["off"]["gain_all"]) - 1, rounds_in_medians=len(per["off"]["wall"]),
                             input="float32 at +/- 1.0, one device tensor [streams, 2, samples], a round = a slice of it; the first "
                                   "round is left out of the medians"),
               frames_per_round=spread(frames),
               switch_off=dict(round_wall_ms=spread(per["off"]["wall"]), append_ms=spread(per["off"]["append"]),
                               gain_ms=spread(per["off"]["gain"])),
               whole_stream=dict(gain_ms=spread(whole), ms_per_second_of_audio=round(statistics.median(whole) / a.seconds, 3)),
               empty_launch_ms=spread(empty), bytes_out=out_bytes)
    if "on" in per:
        total = sum(per["on"]["gain_all"])
        w = statistics.median(whole)
        e = statistics.median(empty)
        doc["switch_on"] = dict(round_wall_ms=spread(per["on"]["wall"]), append_ms=spread(per["on"]["append"]),
                                gain_ms=spread(per["on"]["gain"]), gain_ms_every_round=[round(v, 3) for v in per["on"]["gain_all"]],
                                what="gain_ms_every_round: all rounds in order, the last entry is lamehip_batch_finish's (the flush)")
        doc["one_sample_round_ms"] = spread(tiny)
        doc["rounds_against_whole"] = dict(sum_of_round_gain_ms=round(total, 3), whole_stream_gain_ms=round(w, 3),
                                           difference_ms=round(total - w, 3),
                                           allowed_ms=round(len(per["on"]["gain_all"]) * e + 0.1 * w, 3),
                                           within=bool(total - w <= len(per["on"]["gain_all"]) * e + 0.1 * w),
                                           what="allowed = one empty launch per round + a tenth of the whole-stream time")
        doc["round_wall_on_over_off"] = round(statistics.median(per["on"]["wall"]) / statistics.median(per["off"]["wall"]), 4)
        doc["gains_equal_whole_stream"] = bool(gains == whole_gains)
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
