#!/usr/bin/env python3
"""What device tagging costs a device-packed batch (lamehip_batch_set_device_tagging), and what it saves: the tag kernel's
time against the encode step it runs behind, and the way home of the file images against the host's walk and CRC.

Points: 256 streams x 30 s and (with --big) 1024 streams x 60 s, 44.1 kHz stereo s16, each as CBR 128 and as -V2.  One
process, ONE batch per point whose switch is turned on and off between launches, alternating:

(a) switch on: the tag kernel's HIP-event time (Batch.tag_ms), the audio bytes it read, the time HBM needs for those bytes
    at the rate a copy kernel reaches on this GPU (6.29 TB/s), and the tag kernel as a fraction of the same launch's
    kernel_ms (analysis + sub-band + encode kernels; the tag kernel is not part of it);
(b) switch on: wall clock from the end of lamehip_batch_sync until every image lies in host memory (lamehip_batch_fetch,
    then lamehip_batch_image_ptr of every stream: in place in the pinned buffer);
(c) switch off: the same interval through lamehip_batch_get_bytes_tagged per stream into one reused buffer -- a blocking
    copy, the walk over the frame headers and the table CRC over every byte, as at the parent commit;
(d) switch off: the launch's kernel_ms, and with --baseline-lib PATH a child process that loads the library at PATH (a
    build of the parent commit) and measures the kernel_ms of the same batch there: the two must agree within run-to-run
    noise (tools/ab.sh compares the two builds on the flagship workload).

After one warm-up launch of each kind, `--reps' repetitions; median, min and max of each figure.  Nothing is asserted about
a time; the images of the first streams are checked against the host's.  Writes one JSON document (default
profiles/device_tag_bench.json) and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import lamehip  # noqa: E402

HBM_COPY_RATE = 6.29e12         # bytes / s a float4 copy kernel reaches on the MI355X (8 TB/s on paper)
SETTINGS = (("cbr128", dict(brate=128)), ("V2", dict(vbr_q=2)))


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def open_batch(rate, kw, streams, seconds):
    n = int(rate * seconds)
    base = [helpers.synth_stream(8600 + k, n, rate) for k in range(4)]
    enc = lamehip.Encoder(rate, **kw)
    b = lamehip.Batch(enc, streams, n)
    b.set_device_packing()
    for s in range(streams):
        k, shift = s % len(base), 977 * (s // len(base))
        b.set_pcm(s, np.roll(base[k][0], shift), np.roll(base[k][1], shift))
    return enc, b


def plain_kernel_ms(a, kw):
    """kernel_ms of a batch without the switch, `reps' launches after a warm-up (also what the child of (d) runs)"""
    enc, b = open_batch(a.rate, kw, a.streams, a.seconds)
    out = []
    for rep in range(-1, a.reps):
        b.encode()
        if rep >= 0:
            out.append(b.kernel_ms())
    b.close()
    enc.close()
    return out


def point(a, name, kw, streams, seconds):
    enc, b = open_batch(a.rate, kw, streams, seconds)
    lib = b.lib
    lib.lamehip_batch_get_bytes_tagged.restype = C.c_long
    lib.lamehip_batch_get_bytes_tagged.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    cap = (max(b.frames(s) for s in range(streams)) + 4) * 1500
    buf = C.create_string_buffer(cap)
    tag, on, off, fetch, host, read = [], [], [], [], [], 0
    check = min(4, streams)
    for rep in range(-1, a.reps):
        b.set_device_tagging(True)
        b.encode()
        t0 = time.perf_counter()
        b.fetch()
        sizes = [len(b.image(s)) for s in range(streams)]
        t1 = time.perf_counter()
        images = [bytes(b.image(s)) for s in range(check)]
        tag_ms, on_ms = b.tag_ms(), b.kernel_ms()
        read = sum(len(b.bytes_view(s)) for s in range(streams))
        b.set_device_tagging(False)
        b.encode()
        t2 = time.perf_counter()
        got = []
        for s in range(streams):
            k = lib.lamehip_batch_get_bytes_tagged(b.b, s, buf, cap)
            if k != sizes[s]:
                raise RuntimeError("stream %d: host image %d bytes, device image %d" % (s, k, sizes[s]))
            if s < check:
                got.append(buf.raw[:k])
        t3 = time.perf_counter()
        if got != images:
            raise RuntimeError("the device's images are not the host's")
        if b.tag_ms() != 0:
            raise RuntimeError("the tag kernel ran with the switch off")
        if rep < 0:
            continue
        tag.append(tag_ms)
        on.append(on_ms)
        off.append(b.kernel_ms())
        fetch.append((t1 - t0) * 1000.0)
        host.append((t3 - t2) * 1000.0)
        print("%s %d x %.0f s rep %d: tag kernel %7.3f ms   kernel_ms on %9.3f off %9.3f   images home: fetched %9.2f ms, "
              "by the host's walk and CRC %9.2f ms" % (name, streams, seconds, rep, tag[-1], on[-1], off[-1], fetch[-1], host[-1]),
              flush=True)
    b.close()
    enc.close()
    med_tag = statistics.median(tag)
    hbm_ms = read / HBM_COPY_RATE * 1000.0
    return dict(streams=streams, seconds=seconds, audio_bytes_read=read, tag_kernel_ms=spread(tag),
                hbm_ms_for_those_bytes=round(hbm_ms, 4), tag_kernel_over_hbm_time=round(med_tag / hbm_ms, 2),
                tag_kernel_GB_per_s=round(read / med_tag / 1e6, 1),
                kernel_ms_switch_on=spread(on), kernel_ms_switch_off=spread(off),
                tag_kernel_share_of_the_launch=round(med_tag / statistics.median(on), 5),
                images_home_ms_fetch=spread(fetch), images_home_ms_host_walk_and_crc=spread(host),
                host_over_fetch=round(statistics.median(host) / statistics.median(fetch), 2),
                images_of_first_streams_equal=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="liblamehip.so of the parent commit, for (d)")
    ap.add_argument("--big", action="store_true", help="also 1024 streams x 60 s")
    ap.add_argument("--plain-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_tag_bench.json"))
    a = ap.parse_args()
    if a.plain_child:
        print("PLAIN " + json.dumps(plain_kernel_ms(a, dict(SETTINGS)[a.plain_child])), flush=True)
        return 0
    doc = dict(workload=dict(rate=a.rate, reps=a.reps, input="s16 through the pinned mirror",
                             method="one batch per point, the switch turned on and off between launches, alternating"),
               points={})
    sizes = [(a.streams, a.seconds)] + ([(1024, 60.0)] if a.big else [])
    for streams, seconds in sizes:
        for name, kw in SETTINGS:
            key = "%s_%dx%.0fs" % (name, streams, seconds)
            try:
                doc["points"][key] = point(a, name, kw, streams, seconds)
            except MemoryError as e:
                doc["points"][key] = dict(skipped=str(e)[:200])
    if a.baseline_lib:
        env = dict(os.environ, LAMEHIP_LIB=os.path.abspath(a.baseline_lib))
        for name, kw in SETTINGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--plain-child", name, "--streams", str(a.streams), "--seconds",
                   str(a.seconds), "--rate", str(a.rate), "--reps", str(a.reps)]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("PLAIN ")]
            if r.returncode != 0 or not line:
                raise RuntimeError("baseline child failed:\n" + r.stdout[-2000:])
            parent = json.loads(line[-1][6:])
            p = doc["points"]["%s_%dx%.0fs" % (name, a.streams, a.seconds)]
            p["kernel_ms_parent_commit"] = spread(parent)
            p["kernel_ms_switch_off_over_parent_commit"] = round(p["kernel_ms_switch_off"]["median"] / statistics.median(parent), 4)
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
