#!/usr/bin/env python3
"""What ReplayGain costs a batch (lamehip_batch_set_replaygain): the gain kernel's time against the encode step it runs in
front of, and against the host analysis it replaces.

Default workload: 44.1 kHz stereo s16, CBR 128, 256 streams x 30 s.  One process:

(a) a batch with the switch on, every stream declared again before each launch: the gain kernel's HIP-event time
    (Batch.gain_ms) and the same launch's kernel_ms (analysis + sub-band + encode kernels; the gain kernel is not part of it);
    and, alternating with it, the same launch with LAMEHIP_GAIN_LANES=0 and =1: the gain kernel's two mappings forced (the
    first filter's feedback across the lanes of a row / in lanes 0 and 1; left alone the launch's size
    decides) -- the same sums, other times;
(b) alternating with them, a batch of the same audio with the switch off: its kernel_ms -- what a launch costs when nothing of
    this feature runs;
(c) with --baseline-lib PATH, a child process that loads the library at PATH (a build of the parent commit) and measures
    the kernel_ms of the same batch there: (b) must equal it within run-to-run noise;
(d) the host analysis: lh_rg_block / lh_rg_finish over the same streams in the same blocks (lh_gain_eval_host), `--threads'
    threads (default 16), wall clock -- what the handle API does per stream, and what a batch would have to do without the
    kernel.
With --big the gain kernel and kernel_ms of 1024 streams x 60 s are measured as well (one warm-up, `--reps' repetitions).

After one warm-up launch of each kind, `--reps' repetitions; median, min and max of each figure.  Nothing is asserted about
a time; the gains of the first streams are checked against the host analysis.  Writes one JSON document (default
profiles/replaygain_bench.json) and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers  # noqa: E402
import lamehip  # noqa: E402


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def fill(b, base, streams):
    for s in range(streams):
        k, shift = s % len(base), 977 * (s // len(base))
        b.set_pcm(s, np.roll(base[k][0], shift), np.roll(base[k][1], shift))


def plain_kernel_ms(a):
    """kernel_ms of a batch without the switch, `reps' launches after a warm-up (also what the child of (c) runs)"""
    n = int(a.rate * a.seconds)
    base = [helpers.synth_stream(8600 + k, n, a.rate) for k in range(4)]
    enc = lamehip.Encoder(a.rate, a.brate)
    b = lamehip.Batch(enc, a.streams, n)
    b.set_device_packing()
    fill(b, base, a.streams)
    out = []
    for rep in range(-1, a.reps):
        b.encode()
        if rep >= 0:
            out.append(b.kernel_ms())
    b.close()
    enc.close()
    return out


def host_analysis(lib, base, matrix, streams, rate, threads, fs=1152):
    """the host's analysis of every stream -- lh_gain_eval_host: lh_rg_block over the blocks of lh_gain_plan, a frame's worth
    each and the flush's zeros, then lh_rg_finish -- on `threads' threads; returns (seconds, gains of the first len(base) streams)"""
    lib.lh_gain_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    lib.lh_gain_eval_host.restype = C.c_long
    lib.lh_gain_eval_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p,
                                      C.c_long, C.c_void_p]
    # what the encoder reads: the samples behind the PCM matrix (CBR 128 scales by 0.95), every product and sum a float32
    f = np.float32
    m00, m01, m10, m11 = f(matrix[0]), f(matrix[1]), f(0.0) * f(matrix[0]), f(matrix[2])
    floats = []
    for x in base:
        xl, xr = x[0].astype(np.float32), x[1].astype(np.float32)
        floats.append(np.ascontiguousarray(np.stack([(xl * m00).astype(f) + (xr * m01).astype(f), (xl * m10).astype(f) + (xr * m11).astype(f)]),
                                           dtype=np.float32))
    n = floats[0].shape[1]
    mfn = 1024 + fs - 272
    nb = lib.lh_gain_plan(None, fs, mfn, n, None, 0, None)
    blocks = (C.c_int * nb)()
    assert lib.lh_gain_plan(None, fs, mfn, n, blocks, nb, None) == nb
    gains = [0] * streams

    def work(t):
        for s in range(t, streams, threads):
            x = floats[s % len(base)]
            tenths = C.c_int(0)
            assert lib.lh_gain_eval_host(rate, 2, blocks, nb, x[0].ctypes.data, x[1].ctypes.data, n, None, 0, C.byref(tenths)) >= 0
            gains[s] = tenths.value

    t0 = time.time()
    pool = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    return time.time() - t0, gains[:len(base)]


def gain_point(a, streams, seconds, reps, with_off):
    n = int(a.rate * seconds)
    base = [helpers.synth_stream(8600 + k, n, a.rate) for k in range(4)]
    enc = lamehip.Encoder(a.rate, a.brate)
    cfg = enc.config()
    matrix = (cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r)
    gb = lamehip.Batch(enc, streams, n)
    gb.set_device_packing()
    gb.set_replaygain()
    fill(gb, base, streams)
    pb = None
    if with_off:
        pb = lamehip.Batch(enc, streams, n)
        pb.set_device_packing()
        fill(pb, base, streams)
    gain, lanes, taps, on, off = [], [], [], [], []
    for rep in range(-1, reps):
        forced = {}
        for which in ("1", "0", None):
            if which is None:
                del os.environ["LAMEHIP_GAIN_LANES"]
            else:
                os.environ["LAMEHIP_GAIN_LANES"] = which
            for s in range(streams):
                gb.set_length(s, n)     # declared again: analysed again
            gb.encode()
            forced[which] = (gb.gain_ms(), [gb.radio_gain(s) for s in range(min(4, streams))])
        if not forced["1"][1] == forced["0"][1] == forced[None][1]:
            raise RuntimeError("the two mappings disagree")
        lanes_ms, taps_ms = forced["1"][0], forced["0"][0]
        if pb:
            pb.encode()
        if rep < 0:
            continue
        gain.append(gb.gain_ms())
        lanes.append(lanes_ms)
        taps.append(taps_ms)
        on.append(gb.kernel_ms())
        if pb:
            off.append(pb.kernel_ms())
        print("%d x %.0f s rep %d: gain kernel %8.3f ms (across lanes %8.3f, in lanes 0 and 1 %8.3f)   kernel_ms with the switch on %8.3f%s"
              % (streams, seconds, rep, gain[-1], taps[-1], lanes[-1], on[-1], "   off %8.3f" % off[-1] if pb else ""), flush=True)
    # (streams 0..3 are the four base streams unshifted)
    gains = [gb.radio_gain(s) for s in range(min(4, streams))]
    same = pb is None or all(gb.get_bytes(s) == pb.get_bytes(s) for s in range(min(4, streams)))
    gb.close()
    if pb:
        pb.close()
    enc.close()
    return base, matrix, gain, (taps, lanes), on, off, gains, same


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--brate", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--baseline-lib", default=None, help="liblamehip.so of the parent commit, for (c)")
    ap.add_argument("--big", action="store_true", help="also 1024 streams x 60 s")
    ap.add_argument("--plain-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replaygain_bench.json"))
    a = ap.parse_args()
    if a.plain_child:
        print("PLAIN " + json.dumps(plain_kernel_ms(a)), flush=True)
        return 0

    lib = lamehip.load_library()
    base, matrix, gain, lanes, on, off, gains, same = gain_point(a, a.streams, a.seconds, a.reps, True)
    host_s, host_gains = host_analysis(lib, base, matrix, a.streams, a.rate, a.threads)
    if gains != host_gains[:len(gains)]:
        raise RuntimeError("device gains %s, host gains %s" % (gains, host_gains))
    med_gain, med_off = statistics.median(gain), statistics.median(off)
    doc = dict(workload=dict(rate=a.rate, brate=a.brate, streams=a.streams, seconds=a.seconds, reps=a.reps,
                             input="s16 through the pinned mirror; every stream declared again before each launch"),
               gain_kernel_ms=spread(gain), gain_kernel_ms_taps_across_lanes=spread(lanes[0]),
               gain_kernel_ms_feedback_in_lanes_0_and_1=spread(lanes[1]), kernel_ms_switch_on=spread(on), kernel_ms_switch_off=spread(off),
               gain_kernel_share_of_a_step=round(med_gain / med_off, 4),
               bytes_of_first_streams_equal_on_and_off=bool(same),
               host_analysis=dict(threads=a.threads, seconds=round(host_s, 3), ms=round(host_s * 1000.0, 1),
                                  over_gain_kernel=round(host_s * 1000.0 / med_gain, 2)),
               radio_gain_tenths_db=dict(device=gains, host=host_gains))
    if a.baseline_lib:
        env = dict(os.environ, LAMEHIP_LIB=os.path.abspath(a.baseline_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-child", "--streams", str(a.streams), "--seconds", str(a.seconds),
               "--rate", str(a.rate), "--brate", str(a.brate), "--reps", str(a.reps)]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("PLAIN ")]
        if r.returncode != 0 or not line:
            raise RuntimeError("baseline child failed:\n" + r.stdout[-2000:])
        parent = json.loads(line[-1][6:])
        doc["kernel_ms_parent_commit"] = spread(parent)
        doc["kernel_ms_switch_off_over_parent_commit"] = round(med_off / statistics.median(parent), 4)
    if a.big:
        try:
            _, _, g2, l2, on2, _, _, _ = gain_point(a, 1024, 60.0, a.reps, False)
            doc["streams_1024_x_60_s"] = dict(gain_kernel_ms=spread(g2), gain_kernel_ms_taps_across_lanes=spread(l2[0]),
                                              gain_kernel_ms_feedback_in_lanes_0_and_1=spread(l2[1]),
                                              kernel_ms_switch_on=spread(on2),
                                              gain_kernel_share_of_a_step=round(statistics.median(g2) / statistics.median(on2), 4))
        except (RuntimeError, MemoryError) as e:
            doc["streams_1024_x_60_s"] = dict(skipped=str(e)[:200])
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
