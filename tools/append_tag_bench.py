#!/usr/bin/env python3
"""What carrying the tag frame round by round costs an incremental batch (lamehip_batch_set_incremental_tagging).

Workload: tools/append_packing_bench.py's -- 44.1 kHz, 256 streams x 30 s, float32 at +/- 1.0 from a device tensor in
rounds of one second (lamehip_batch_append_device) --, at CBR 128 and at -V2.  One process; two batches that pack their
rounds on the device are fed the same tensor and take turns round by round, one with the switch on, one with it off.

  per round: Batch.tag_ms(), the one launch of lh_tag_resume_kernel, next to the same round's Batch.drain_ms(), the three
      launches of csrc/lh_drain.hip; and the wall time of append_device + encode_available + the drain of every stream
      with the switch on and off;
  the tag launches summed over all rounds, the final one included, against the one-shot lh_tag_kernel
      (lamehip_batch_set_device_tagging) of a whole-stream batch fed the same samples: the same bytes read once either way;
  the time from the end of finish() -- the final round's wait -- until every tag lies in host memory (tags_all()), against
      making the tags on the host from the concatenated drains: lh_tag_crc over every byte, and a walk over the frame
      headers that feeds lh_tag_add_frame, then lh_tag_frame.  The walk is a Python loop here and is reported apart from
      the CRC, which is C and so the fair lower bound of the host's route.

The first round (allocations, nothing to encode yet) is left out of the per-round figures; median, min and max over the
others.  The tags are compared with the one-shot batch's and with the host's; nothing is asserted about a time.  Writes
one JSON document (default profiles/append_tag_bench.json) and prints it."""
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
from ingest_bench import spread, typed  # noqa: E402
from test_device_tag import LhVbrTag  # noqa: E402


def host_tags(lib, enc, streams):
    """the tags made on the host from every stream's audio bytes; returns (tags, ms of the CRC, ms of the header walk)"""
    cfg = enc.config()
    lib.lh_tag_crc.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.lh_tag_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    factor = (cfg.version + 1) * 72000
    kbps = [lib.lh_tag_kbps(cfg.version, i) for i in range(16)]
    tags, crc_s, walk_s = [], 0.0, 0.0
    for audio, nsamples in streams:
        v = LhVbrTag()
        total = lib.lh_tag_init(C.byref(v), C.byref(cfg))
        t0 = time.perf_counter()
        lib.lh_tag_crc(C.byref(v), audio, len(audio))
        t1 = time.perf_counter()
        pos, ext = 0, 0
        while pos + 4 <= len(audio):
            b2 = audio[pos + 2]
            lib.lh_tag_add_frame(C.byref(v), kbps[b2 >> 4])
            ext = (audio[pos + 3] >> 4) & 3
            pos += factor * kbps[b2 >> 4] // cfg.samplerate + ((b2 >> 1) & 1)
        t2 = time.perf_counter()
        out = C.create_string_buffer(total)
        pad = lib.lh_end_padding_fs(C.c_long(nsamples), 576 * cfg.mode_gr)
        assert lib.lh_tag_frame(C.byref(v), C.byref(cfg), cfg.vbr_q, pad, ext, out, total) == total
        tags.append(out.raw)
        crc_s += t1 - t0
        walk_s += t2 - t1
    return tags, crc_s * 1e3, walk_s * 1e3


def one_setting(a, lib, name, kw, dev_base, dev_kind, dev_plane, dev_shift, n, T):
    B = a.streams
    stype = lamehip.PCM_F32_UNIT
    enc = lamehip.Encoder(a.rate, **kw)
    batches = {}
    for mode in ("on", "off"):
        b = lamehip.Batch(enc, B, n)
        b.set_sample_type(stype)
        b.set_device_packing()
        b.set_incremental_packing()
        if mode == "on":
            b.set_incremental_tagging()
        batches[mode] = b
    on = batches["on"]
    size = on.tag_size()
    wall = dict(on=[], off=[])
    tag_ms, drain_ms, kern_ms, tag_sum = [], [], [], 0.0
    audio = [[] for _ in range(B)]
    same = True
    whole = torch.empty((B, 2, n), dtype=torch.float32, device="cuda:0")
    for rnd, pos in enumerate(range(0, n, T)):
        m = min(T, n - pos)
        idx = (dev_shift + pos + torch.arange(m, device="cuda:0")[None, :]) % n
        chunk = dev_base[dev_kind, dev_plane, idx[:, None, :]].contiguous()
        whole[:, :, pos:pos + m] = chunk
        torch.cuda.synchronize()
        got = {}
        # (the two modes take turns in going first)
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
        for s in range(B):
            audio[s].append(got["on"][s])
        tag_sum += on.tag_ms()
        if rnd == 0 or m < T:
            continue
        tag_ms.append(on.tag_ms())
        drain_ms.append(on.drain_ms())
        kern_ms.append(on.kernel_ms())
        print("%s round %2d: switch on %7.2f ms, off %7.2f ms   encode kernels %7.2f ms, drain %6.3f ms, tag %6.3f ms"
              % (name, rnd, wall["on"][-1], wall["off"][-1], kern_ms[-1], drain_ms[-1], tag_ms[-1]), flush=True)
    batches["off"].finish()
    fin_off = [batches["off"].drain_view(s).tobytes() for s in range(B)]
    on.finish()
    t0 = time.perf_counter()
    out, sizes = on.tags_all()
    t1 = time.perf_counter()
    final_tag_ms = on.tag_ms()
    tag_sum += final_tag_ms
    fin_on = [on.drain_view(s).tobytes() for s in range(B)]
    same = same and fin_on == fin_off
    streams = [(b"".join(audio[s]) + fin_on[s], n) for s in range(B)]
    tags = [bytes(out[s, :sizes[s]]) for s in range(B)]
    by_host, crc_ms, walk_ms = host_tags(lib, enc, streams)
    for b in batches.values():
        b.close()
    # the one-shot batch over the same samples: its tag kernel's time, and its tags
    one = lamehip.Batch(enc, B, n)
    one.set_device_packing()
    one.set_device_tagging()
    one.set_sample_type(stype)
    for s in range(B):
        one.set_input(s, whole[s, 0], whole[s, 1])
    shot_ms = []
    for rep in range(3):
        one.encode()
        shot_ms.append(one.tag_ms())
    one.fetch()
    by_one_shot = [bytes(one.image(s)[:size]) for s in range(B)]
    one.close()
    enc.close()
    med = statistics.median
    return dict(settings=kw, tag_size=size, rounds_measured=len(tag_ms), audio_bytes=sum(len(x[0]) for x in streams),
                per_round=dict(tag_ms=spread(tag_ms), drain_ms=spread(drain_ms), encode_kernels_ms=spread(kern_ms),
                               tag_over_drain=round(med(tag_ms) / med(drain_ms), 3),
                               tag_share_of_the_encode_kernels=round(med(tag_ms) / med(kern_ms), 5)),
                final_round_tag_ms=round(final_tag_ms, 4),
                tag_ms_summed_over_all_rounds=round(tag_sum, 4),
                one_shot_tag_kernel_ms=spread(shot_ms),
                summed_over_one_shot=round(tag_sum / med(shot_ms), 2),
                tags_home_after_finish_ms=round((t1 - t0) * 1e3, 4),
                tags_on_the_host_from_the_drains_ms=dict(crc_in_c=round(crc_ms, 2), header_walk_in_python=round(walk_ms, 2)),
                host_crc_alone_over_tags_home=round(crc_ms / ((t1 - t0) * 1e3), 1),
                round_wall_ms=dict(switch_on=spread(wall["on"]), switch_off=spread(wall["off"]),
                                   on_over_off=round(med(wall["on"]) / med(wall["off"]), 4)),
                drains_equal_with_the_switch_on_and_off=bool(same),
                tags_equal_the_one_shot_batch=bool(tags == by_one_shot), tags_equal_the_host=bool(tags == by_host))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--round-seconds", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_tag_bench.json"))
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
    doc = dict(workload=dict(rate=a.rate, streams=B, seconds=a.seconds, round_seconds=a.round_seconds,
                             input="float32 at +/- 1.0, [streams, 2, samples of a round] on the device; first round left out of the "
                                   "per-round figures; the two batches take turns within a round",
                             round="append_device + encode_available + the drain of every stream (in place)"),
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
