"""Child process of tests/test_incremental_packing_device.py::test_conversion_and_replaygain_on_top_fed_from_a_tensor: torch
takes the device first, then eight float32 streams at +/- 1.0 -- held as one tensor [B, 2, cap] on the same GPU, NaN beyond
each length -- are fed round by round through append_device, ragged lengths and 0, to two incremental batches that convert
48 -> 44.1 kHz and measure ReplayGain round by round: one on the host packer, one with lamehip_batch_set_incremental_packing.
After every round the drains are equal, after finish the radio gains."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHUNKS = [0, 1, 3, 575, 1152, 1153, 4000, 9000]


def main():
    torch.zeros(1, device="cuda:0")
    import lamehip
    import pcm_input_support as psup
    import test_pcm_input_device as t
    stype, sr, out, kw, B = lamehip.PCM_F32_UNIT, 48000, 44100, dict(brate=128), 8
    lens = [int(0.9 * sr) + 37 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9990 + s, lens[s], sr) for s in range(B)]
    cap = max(lens) + 2
    host = np.full((B, 2, cap), np.nan, np.float32)
    for s, x in enumerate(xs):
        host[s, :, :lens[s]] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    enc = t.open_product(sr, kw, out)
    batches = []
    for packing in (False, True):
        b = lamehip.Batch(enc, B, cap)
        b.set_device_resampling()
        b.set_sample_type(stype)
        if packing:
            b.set_device_packing()
            b.set_incremental_packing()
        b.set_incremental_resampling()
        b.set_incremental_replaygain()
        batches.append(b)
    rng = np.random.default_rng(98)
    pos, rnd, total, ms = [0] * B, 0, 0, 0.0
    while any(pos[s] < lens[s] for s in range(B)):
        ns = [min(int(rng.choice(CHUNKS)), lens[s] - pos[s]) for s in range(B)]
        T = max(ns) + 5
        chunk = torch.full((B, 2, T), float("nan"), device="cuda:0")
        for s in range(B):
            chunk[s, :, :ns[s]] = dev[s, :, pos[s]:pos[s] + ns[s]]
        torch.cuda.synchronize()                                        # the producer has finished
        for b in batches:
            b.append_device(chunk, ns)
        chunk.fill_(float("nan"))                                       # reusable at once
        assert batches[0].encode_available() == batches[1].encode_available()
        ms += batches[1].drain_ms()
        for s in range(B):
            got = batches[1].drain(s)
            assert got == batches[0].drain(s), "round %d stream %d" % (rnd, s)
            total += len(got)
            pos[s] += ns[s]
        rnd += 1
    assert batches[0].finish() == batches[1].finish()
    for s in range(B):
        got = batches[1].drain(s)
        assert got == batches[0].drain(s), "flush of stream %d" % s
        total += len(got)
        assert batches[1].radio_gain(s) == batches[0].radio_gain(s), s
    assert rnd > 3 and total > B * 10000 and ms > 0.0
    for b in batches:
        b.close()
    enc.close()
    print("incremental packing ok: %d rounds, %d bytes" % (rnd, total), flush=True)


if __name__ == "__main__":
    main()
