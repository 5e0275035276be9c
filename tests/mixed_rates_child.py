"""Child process of tests/test_mixed_rates_device.py (test_float32_from_a_torch_tensor): torch takes the device first, then
four float32 streams at +/- 1.0 and at four input rates -- held as one tensor [B, 2, cap] on the same GPU, NaN beyond each
length -- are fed to one incremental batch that converts to 44.1 kHz, one append_device per round with ragged lengths
(the chunks of tests/mixed_rates_support.py, then 9000 at a time).  What every stream drains after a round must be what
lame_encode_buffer_ieee_float returned for that call at (in = the stream's rate, out = 44.1 kHz)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    torch.zeros(1, device="cuda:0")
    import lamehip
    import pcm_input_support as psup
    import test_append_resample_device as tard
    import test_mixed_rates_device as tm
    import test_pcm_input_device as t
    stype, own, out, kw = lamehip.PCM_F32_UNIT, 48000, 44100, dict(brate=128, mode=1)
    rates = [32000, 48000, 44100, 8000]
    B = len(rates)
    lens = [int(0.35 * hz) + 29 * s for s, hz in enumerate(rates)]
    xs = [psup.typed_signal(stype, 8700 + s, lens[s], hz) for s, hz in enumerate(rates)]
    cap = max(lens) + 2
    host = np.full((B, 2, cap), np.nan, np.float32)
    for s, x in enumerate(xs):
        host[s, :, :lens[s]] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    eps = [tard.EntryPoint(stype, False, hz, kw, out) for hz in rates]
    enc = t.open_product(own, kw, out)
    b = tm.open_pool(enc, stype, B, cap)
    for s, hz in enumerate(rates):
        b.set_stream_in_samplerate(s, hz)
    calls = [tm.calls_of(lens[s], s) for s in range(B)]
    pos, rounds = [0] * B, max(len(c) for c in calls)
    for rnd in range(rounds):
        ns = [calls[s][rnd] if rnd < len(calls[s]) else 0 for s in range(B)]
        T = max(max(ns), 1)
        chunk = torch.full((B, 2, T), float("nan"), device="cuda:0")
        for s in range(B):
            chunk[s, :, :ns[s]] = dev[s, :, pos[s]:pos[s] + ns[s]]
        torch.cuda.synchronize()                                        # the producer has finished
        b.append_device(chunk, ns)
        b.encode_available()
        for s in range(B):
            want = eps[s].call(xs[s][:, pos[s]:pos[s] + ns[s]])
            assert b.drain(s) == want, "round %d stream %d (%d Hz)" % (rnd, s, rates[s])
            pos[s] += ns[s]
    b.finish()
    for s in range(B):
        flush = eps[s].flush()
        assert b.drain(s) == flush and len(flush) > 0, "flush of stream %d (%d Hz)" % (s, rates[s])
    b.close()
    enc.close()
    print("mixed rates ok: %d rounds" % rounds, flush=True)


if __name__ == "__main__":
    main()
