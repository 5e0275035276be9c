#!/usr/bin/env python3
"""What packing an incremental batch's rounds on the device costs or saves (lamehip_batch_set_incremental_packing).

Workload: tools/append_bench.py's -- 44.1 kHz, 256 streams x 30 s, float32 at +/- 1.0 from a device tensor in rounds of
one second (lamehip_batch_append_device) --, at CBR 128 and at -V2.  One process; two batches fed the same tensor take
turns round by round, one on the host packer, one with the switch on.  Per round:

  wall time of append_device + encode_available + the drain of every stream, in both modes (the host-packed batch through
      drain, which copies; the device-packed one through drain_view, which does not);
  the encode kernels' ms (Batch.kernel_ms) in both modes -- with the switch on they include the bit packer's work;
  Batch.drain_ms(): the three launches of csrc/lh_drain.hip;
  the bytes the round gathered, and the bytes that crossed to the host: frames x sizeof(LhFrameOut) against the table plus
      the gathered bytes;
  as a yardstick for the gather, the runtime's device-to-device copy of the same byte count, between events on a stream of
      its own.

The first round (allocations, nothing to encode yet) is left out; median, min and max over the others.  The two modes'
bytes are compared; nothing is asserted about a time.  Writes one JSON document (default
profiles/append_packing_bench.json) and prints it."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import helpers  # noqa: E402
import lamehip  # noqa: E402
from ingest_bench import DeviceCopy, spread, typed  # noqa: E402

ROW_BYTES = 40          # sizeof(LhDrainRow), csrc/lh_drain.h


def one_setting(a, lib, name, kw, dev_base, dev_kind, dev_plane, dev_shift, n, T):
    B = a.streams
    stype = lamehip.PCM_F32_UNIT
    enc = lamehip.Encoder(a.rate, **kw)
    frame_out = lib.lamehip_abi_sizeof(2)     # sizeof(LhFrameOut)
    hb = lamehip.Batch(enc, B, n)
    hb.set_sample_type(stype)
    db = lamehip.Batch(enc, B, n)
    db.set_sample_type(stype)
    db.set_device_packing()
    db.set_incremental_packing()
    copy = DeviceCopy(lib, 64 << 20)
    wall = dict(host=[], device=[])
    kern = dict(host=[], device=[])
    drain_ms, gathered, copies, frames, home_host, home_dev = [], [], [], [], [], []
    out = dict(host=0, device=0)
    same = True
    for rnd, pos in enumerate(range(0, n, T)):
        m = min(T, n - pos)
        idx = (dev_shift + pos + torch.arange(m, device="cuda:0")[None, :]) % n
        chunk = dev_base[dev_kind, dev_plane, idx[:, None, :]].contiguous()
        torch.cuda.synchronize()
        got = {}
        # (the two modes take turns in going first)
        for mode in (("host", "device") if rnd % 2 else ("device", "host")):
            b = hb if mode == "host" else db
            t0 = time.perf_counter()
            b.append_device(chunk, [m] * B)
            k = b.encode_available()
            if mode == "host":
                got[mode] = [b.drain(s) for s in range(B)]
            else:
                got[mode] = [b.drain_view(s).tobytes() if a.check else bytes(len(b.drain_view(s))) for s in range(B)]
            t1 = time.perf_counter()
            if rnd > 0 and m == T:
                wall[mode].append((t1 - t0) * 1e3)
                kern[mode].append(b.kernel_ms())
            out[mode] += sum(len(x) for x in got[mode])
        if a.check:
            same = same and got["host"] == got["device"]
        nbytes = sum(len(x) for x in got["device"])
        c = copy.run(nbytes) if nbytes else 0.0
        if rnd == 0 or m < T:
            continue
        drain_ms.append(db.drain_ms())
        gathered.append(nbytes)
        copies.append(c)
        frames.append(k)
        home_host.append(k * frame_out)
        home_dev.append(ROW_BYTES * (B + 1) + (nbytes + 15 * B) // 16 * 16)
        print("%s round %2d: host packer %7.2f ms (kernels %7.2f)   device packer %7.2f ms (kernels %7.2f, drain %6.3f, copy of the "
              "same bytes %6.3f)   %d frames, %d bytes" % (name, rnd, wall["host"][-1], kern["host"][-1], wall["device"][-1],
                                                           kern["device"][-1], drain_ms[-1], c, k, nbytes), flush=True)
    hb.finish()
    db.finish()
    fin = [hb.drain(s) for s in range(B)], [db.drain_view(s).tobytes() for s in range(B)]
    same = same and fin[0] == fin[1]
    out["host"] += sum(len(x) for x in fin[0])
    out["device"] += sum(len(x) for x in fin[1])
    copy.close()
    hb.close()
    db.close()
    enc.close()
    med = statistics.median
    return dict(settings=kw, rounds_measured=len(drain_ms), frames_per_round=spread(frames),
                round_wall_ms=dict(host_packer=spread(wall["host"]), device_packer=spread(wall["device"]),
                                   device_over_host=round(med(wall["device"]) / med(wall["host"]), 4)),
                encode_kernels_ms=dict(host_packer=spread(kern["host"]), device_packer=spread(kern["device"]),
                                       device_over_host=round(med(kern["device"]) / med(kern["host"]), 4)),
                drain_ms=spread(drain_ms), bytes_gathered=spread(gathered),
                copy_of_the_same_bytes_ms=spread(copies), drain_over_copy=round(med(drain_ms) / med(copies), 3),
                bytes_to_host_per_round=dict(host_packer=spread(home_host), device_packer=spread(home_dev),
                                             host_over_device=round(med(home_host) / med(home_dev), 2)),
                bytes_out=out, bytes_equal=bool(same) if a.check else "final round only: %r" % bool(same))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--round-seconds", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--no-check", dest="check", action="store_false", help="do not compare the two modes' bytes round by round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_packing_bench.json"))
    a = ap.parse_args()

    torch.zeros(1, device="cuda:0")                             # torch takes the device first
    B, n, T = a.streams, int(a.rate * a.seconds), int(a.rate * a.round_seconds)
    stype = lamehip.PCM_F32_UNIT
    xs = [typed(stype, helpers.synth_stream(8800 + k, n, a.rate)) for k in range(4)]
    kind = np.arange(B) % len(xs)
    shift = 977 * (np.arange(B) // len(xs))
    dev_base = torch.from_numpy(np.stack(xs)).to("cuda:0")      # [4, 2, n]
    dev_kind = torch.from_numpy(kind).to("cuda:0")[:, None, None]
    dev_plane = torch.arange(2, device="cuda:0")[None, :, None]
    dev_shift = torch.from_numpy(shift).to("cuda:0")[:, None]
    lib = lamehip.load_library()
    lib.lamehip_abi_sizeof.argtypes = [C.c_int]
    doc = dict(workload=dict(rate=a.rate, streams=B, seconds=a.seconds, round_seconds=a.round_seconds,
                             input="float32 at +/- 1.0, [streams, 2, samples of a round] on the device; first round left out; the two "
                                   "batches take turns within a round",
                             round="append_device + encode_available + the drain of every stream"),
               settings={})
    for name, kw in (("cbr128", dict(brate=128)), ("vbr2", dict(vbr_q=2))):
        doc["settings"][name] = one_setting(a, lib, name, kw, dev_base, dev_kind, dev_plane, dev_shift, n, T)
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
