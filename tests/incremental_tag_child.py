"""Child process of tests/test_incremental_tag_device.py::test_conversion_on_top_fed_from_a_tensor: torch takes the device
first, then eight float32 streams at +/- 1.0 -- held as one tensor [B, 2, cap] on the same GPU, NaN beyond each length -- are
fed round by round through append_device, ragged lengths and 0, to an incremental batch that converts 48 -> 44.1 kHz round by
round, packs on the device and carries tag frames (lamehip_batch_set_incremental_tagging).  After finish every stream's tag
and image are those of the one-shot batch that converts, packs and tags on the device."""
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
    xs = [psup.typed_signal(stype, 9460 + s, lens[s], sr) for s in range(B)]
    cap = max(lens) + 2
    host = np.full((B, 2, cap), np.nan, np.float32)
    for s, x in enumerate(xs):
        host[s, :, :lens[s]] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    enc = t.open_product(sr, kw, out)
    one = t.typed_batch(enc, stype, B, cap, dev_rs=True)
    one.set_device_tagging()
    t.feed(one, xs, False, False)
    one.encode()
    images = [one.get_bytes_tagged(s) for s in range(B)]
    one.close()
    b = lamehip.Batch(enc, B, cap)
    b.set_device_resampling()
    b.set_sample_type(stype)
    b.set_device_packing()
    b.set_incremental_packing()
    b.set_incremental_resampling()
    b.set_incremental_tagging()
    T = b.tag_size()
    assert T > 0
    rng = np.random.default_rng(99)
    pos, rnd, drained, ms = [0] * B, 0, [b""] * B, 0.0
    while any(pos[s] < lens[s] for s in range(B)):
        ns = [min(int(rng.choice(CHUNKS)), lens[s] - pos[s]) for s in range(B)]
        chunk = torch.full((B, 2, max(ns) + 5), float("nan"), device="cuda:0")
        for s in range(B):
            chunk[s, :, :ns[s]] = dev[s, :, pos[s]:pos[s] + ns[s]]
            pos[s] += ns[s]
        torch.cuda.synchronize()                                        # the producer has finished
        b.append_device(chunk, ns)
        b.encode_available()
        ms += b.tag_ms()
        for s in range(B):
            drained[s] += b.drain(s)
        rnd += 1
    b.finish()
    for s in range(B):
        drained[s] += b.drain(s)
        tag = b.tag(s)
        assert tag == images[s][:T], "tag of stream %d" % s
        assert tag + drained[s] == images[s], "image of stream %d" % s
    assert rnd > 3 and ms > 0.0
    b.close()
    enc.close()
    print("incremental tagging ok: %d rounds, %d bytes of tags" % (rnd, B * T), flush=True)


if __name__ == "__main__":
    main()
