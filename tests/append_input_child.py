"""Child process of tests/test_append_input_device.py::test_device_resident_appends_from_torch: torch takes the device first,
then the streams -- float32 at +/- 1.0, held as one tensor [B, 2, cap] on the same GPU, NaN beyond each length -- are fed to
incremental batches round by round: once through Batch.append_device (one launch per round, ragged lengths and 0, the
round's chunks as a tensor of their own, as a view of a larger one and interleaved), once per stream through
Batch.append_input with tensor slices, host arrays on alternate rounds.  The drains, concatenated, must be pack(s) of the
one-shot typed batch, and converted(s) the host evaluation's floats."""
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
    import test_append_input_device as ta
    import test_pcm_input_device as t
    stype, sr, kw, B = lamehip.PCM_F32_UNIT, 44100, dict(brate=128), 8
    lens = [int(0.6 * sr) + 37 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9700 + s, lens[s], sr) for s in range(B)]
    cap = max(lens) + 2
    host = np.full((B, 2, cap), np.nan, np.float32)
    for s, x in enumerate(xs):
        host[s, :, :lens[s]] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    enc = t.open_product(sr, kw)
    want = ta.one_shot(enc, stype, xs, cap)
    for how in ("append_device", "append_input"):
        rng = np.random.default_rng(97)
        b = lamehip.Batch(enc, B, cap)
        b.set_sample_type(stype)
        got = [b""] * B
        pos, rnd, ms = [0] * B, 0, 0.0
        while any(pos[s] < lens[s] for s in range(B)):
            ns = [min(int(rng.choice(CHUNKS)), lens[s] - pos[s]) for s in range(B)]
            if how == "append_device":
                # the round's chunks as the producer would hold them: [B, 2, T], NaN where a stream has nothing
                T = max(ns) + 5
                big = torch.full((B, 2, T + 9), float("nan"), device="cuda:0")
                chunk = big[:, :, 3:3 + T] if rnd % 3 == 1 else torch.full((B, 2, T), float("nan"), device="cuda:0")
                for s in range(B):
                    chunk[s, :, :ns[s]] = dev[s, :, pos[s]:pos[s] + ns[s]]
                if rnd % 3 == 2:
                    chunk = chunk.permute(0, 2, 1).contiguous()         # [B, T, 2]
                torch.cuda.synchronize()                                # the producer has finished
                b.append_device(chunk, ns)
                if max(ns) > 0:
                    assert b.append_ms() > 0.0
                    ms += b.append_ms()
                chunk.fill_(float("nan"))                               # reusable at once
            else:
                for s in range(B):
                    a, e = pos[s], pos[s] + ns[s]
                    m = a + ns[s] // 2
                    if (rnd + s) % 2:
                        b.append_input(s, dev[s, 0, a:e], dev[s, 1, a:e])
                    else:
                        # (staged first, then a device-resident chunk behind it: the places are fixed when they are appended)
                        b.append_input(s, xs[s][0, a:m], xs[s][1, a:m])
                        pairs = dev[s, :, m:e].t().contiguous()         # [n, 2]
                        torch.cuda.synchronize()
                        b.append_input(s, interleaved=pairs)
            for s in range(B):
                pos[s] += ns[s]
            b.encode_available()
            ta.drain_all(b, got)
            rnd += 1
        b.finish()
        ta.drain_all(b, got)
        for s in range(B):
            assert got[s] == want[s], (how, s)
        t.check_floats(b, enc, stype, xs)
        assert rnd > 3 and (how != "append_device" or ms > 0.0)
        b.close()
        print("device-resident append ok: %s, %d rounds" % (how, rnd), flush=True)
    enc.close()


if __name__ == "__main__":
    main()
