#!/usr/bin/env python3
"""What typed input costs a batch (lamehip_batch_set_sample_type): the ingest kernel against the runtime's own copy, and
the front kernels reading the float pool against reading s16.

Default workload: 44.1 kHz, CBR 128, 256 streams x 30 s, for PCM_F32_UNIT and PCM_S32.  One process, per sample type:

(a) the ingest kernel's HIP-event time (Batch.ingest_ms: every stream declared again before each launch) and, alternating
    with it, a hipMemcpyAsync device-to-device between two scratch buffers, timed with HIP events on a stream of its own --
    once of as many bytes as the kernel reads plus writes (the yardstick), once of as many bytes as it reads (a copy that
    moves the kernel's own traffic: the pool read, as much written).  Expectation on record: the kernel within 1.5 x of
    the yardstick copy -- the same kind of traffic with one multiply-add pair per sample, over ragged rows.
(b) kernel_parts_ms (analysis, sub-band, encode) of the typed batch against an s16 batch of the same audio rounded to
    int16, alternating: the float pool goes through the front kernels' plain float staging loop, not the wide s16 path.

After one warm-up launch of each kind, `--reps' repetitions; median, min and max of each figure.  Nothing is asserted about
a time.  Writes one JSON document (default profiles/ingest_bench.json) and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import lamehip  # noqa: E402

HBM_PEAK_GBS = 8000.0           # MI355X HBM3E, 8 TB/s
D2D = 3                         # hipMemcpyDeviceToDevice


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


class DeviceCopy:
    """hipMemcpyAsync device-to-device between two scratch buffers, between two events on its own stream"""

    def __init__(self, lib, nbytes):
        self.lib, self.nbytes = lib, nbytes
        for name, args in (("hipMalloc", [C.c_void_p, C.c_size_t]), ("hipFree", [C.c_void_p]), ("hipMemset", [C.c_void_p, C.c_int, C.c_size_t]),
                           ("hipStreamCreate", [C.c_void_p]), ("hipStreamDestroy", [C.c_void_p]), ("hipStreamSynchronize", [C.c_void_p]),
                           ("hipEventCreate", [C.c_void_p]), ("hipEventDestroy", [C.c_void_p]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                           ("hipEventElapsedTime", [C.c_void_p, C.c_void_p, C.c_void_p]),
                           ("hipMemcpyAsync", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p])):
            getattr(lib, name).argtypes = args
        self.src, self.dst, self.stream, self.e0, self.e1 = (C.c_void_p() for _ in range(5))
        self.ok(lib.hipMalloc(C.byref(self.src), nbytes))
        self.ok(lib.hipMalloc(C.byref(self.dst), nbytes))
        self.ok(lib.hipMemset(self.src, 1, nbytes))
        self.ok(lib.hipMemset(self.dst, 2, nbytes))
        self.ok(lib.hipStreamCreate(C.byref(self.stream)))
        self.ok(lib.hipEventCreate(C.byref(self.e0)))
        self.ok(lib.hipEventCreate(C.byref(self.e1)))

    @staticmethod
    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP call failed (%d)" % rc)

    def run(self, nbytes):
        assert nbytes <= self.nbytes
        ms = C.c_float(0)
        self.ok(self.lib.hipEventRecord(self.e0, self.stream))
        self.ok(self.lib.hipMemcpyAsync(self.dst, self.src, nbytes, D2D, self.stream))
        self.ok(self.lib.hipEventRecord(self.e1, self.stream))
        self.ok(self.lib.hipStreamSynchronize(self.stream))
        self.ok(self.lib.hipEventElapsedTime(C.byref(ms), self.e0, self.e1))
        return float(ms.value)

    def close(self):
        self.lib.hipEventDestroy(self.e0)
        self.lib.hipEventDestroy(self.e1)
        self.lib.hipStreamDestroy(self.stream)
        self.lib.hipFree(self.src)
        self.lib.hipFree(self.dst)


def typed(stype, base):
    """the s16 stream `base' plus a fraction of a step, in the sample type's scale"""
    rng = np.random.Generator(np.random.PCG64(stype))
    x = base.astype(np.float64) + rng.uniform(-0.4, 0.4, base.shape)
    if stype == lamehip.PCM_F32_UNIT:
        x = x / 32767.0
    if stype == lamehip.PCM_S32:
        x = x * 65536.0
    return np.ascontiguousarray(x.astype(lamehip.PCM_DTYPES[stype]))


def rounded(stype, x):
    """the typed stream rounded to int16: what a producer without typed input would hand over"""
    scale = {lamehip.PCM_F32_UNIT: 32767.0, lamehip.PCM_S32: 1.0 / 65536.0}.get(stype, 1.0)
    return np.rint(x.astype(np.float64) * scale).clip(-32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--brate", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    a = ap.parse_args()

    n = int(a.rate * a.seconds)
    base = [helpers.synth_stream(8600 + k, n, a.rate) for k in range(4)]
    lib = lamehip.load_library()
    enc = lamehip.Encoder(a.rate, a.brate)
    doc = dict(workload=dict(rate=a.rate, brate=a.brate, streams=a.streams, seconds=a.seconds, reps=a.reps,
                             input="through the pinned mirror; every stream declared again before each launch"),
               hbm_peak_gb_per_s=HBM_PEAK_GBS, types={})
    for stype in (lamehip.PCM_F32_UNIT, lamehip.PCM_S32):
        name = {lamehip.PCM_F32_UNIT: "f32_unit", lamehip.PCM_S32: "s32"}[stype]
        xs = [typed(stype, b) for b in base]
        rs = [rounded(stype, x) for x in xs]
        tb = lamehip.Batch(enc, a.streams, n)
        tb.set_device_packing()
        tb.set_sample_type(stype)
        sb = lamehip.Batch(enc, a.streams, n)
        sb.set_device_packing()
        for s in range(a.streams):
            k, shift = s % len(xs), 977 * (s // len(xs))
            tb.set_input(s, np.roll(xs[k][0], shift), np.roll(xs[k][1], shift))
            sb.set_pcm(s, np.roll(rs[k][0], shift), np.roll(rs[k][1], shift))
        pool_bytes = a.streams * 2 * n * 4                      # read by the kernel; it writes as much
        copy = DeviceCopy(lib, 2 * pool_bytes)
        ingest, copy_rw, copy_r, parts_t, parts_s = [], [], [], [], []
        for rep in range(-1, a.reps):                           # (-1: warm-up)
            for s in range(a.streams):
                tb.set_length(s, n)
            tb.encode()
            c_rw, c_r = copy.run(2 * pool_bytes), copy.run(pool_bytes)
            sb.encode()
            if rep < 0:
                continue
            ingest.append(tb.ingest_ms())
            copy_rw.append(c_rw)
            copy_r.append(c_r)
            parts_t.append(tb.kernel_parts_ms()[1])
            parts_s.append(sb.kernel_parts_ms()[1])
            print("%-8s rep %d: ingest %7.3f ms   copy of read + written bytes %7.3f ms, of read bytes %7.3f ms   parts typed %s   s16 %s"
                  % (name, rep, ingest[-1], c_rw, c_r, ["%.2f" % v for v in parts_t[-1]], ["%.2f" % v for v in parts_s[-1]]), flush=True)
        differ = sum(tb.get_bytes(s) != sb.get_bytes(s) for s in range(min(4, a.streams)))
        copy.close()
        tb.close()
        sb.close()
        med = statistics.median(ingest)
        doc["types"][name] = dict(
            ingest_ms=spread(ingest), bytes_read=pool_bytes, bytes_written=pool_bytes,
            ingest_gb_per_s=round(2 * pool_bytes / med / 1e6, 1), ingest_share_of_hbm_peak=round(2 * pool_bytes / med / 1e6 / HBM_PEAK_GBS, 4),
            copy_of_read_plus_written_bytes_ms=spread(copy_rw), copy_of_read_bytes_ms=spread(copy_r),
            ingest_over_copy_of_read_plus_written_bytes=round(med / statistics.median(copy_rw), 3),
            ingest_over_copy_of_read_bytes=round(med / statistics.median(copy_r), 3),
            expectation="ingest within 1.5 x of the copy of read + written bytes",
            kernel_parts_ms_typed=dict(zip(("analysis", "subband", "encode"), (spread([p[i] for p in parts_t]) for i in range(3)))),
            kernel_parts_ms_s16=dict(zip(("analysis", "subband", "encode"), (spread([p[i] for p in parts_s]) for i in range(3)))),
            streams_of_4_whose_bytes_differ_from_the_rounded_s16=differ)
    enc.close()
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
