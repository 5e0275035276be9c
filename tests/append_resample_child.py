"""Child process of tests/test_append_resample_device.py (test_mixed_sources_from_torch, test_launches_in_windows): torch
takes the device first, then four float32 streams at +/- 1.0 -- held as one tensor [B, 2, cap] on the same GPU, NaN beyond
each length -- are fed to an incremental batch that converts 48 -> 44.1 kHz, 1152 samples per append, one append per stream
and round (five with the argument `window').  The appends take turns: append_device from a [B, 2, T] tensor of the round's chunks, from a view of a larger one, from an interleaved
[B, T, 2] one -- there one stream of each pair has nothing in the tensor and is fed from host arrays --, and per stream
through append_input with tensor slices (append_input_device) for one stream of each pair and host arrays for the other.
The drains, concatenated, must be pack(s) of the one-shot whole-stream batch of the same samples, whose plan is the
reference fed 1152 samples per call, and converted(s) its floats.  Argument `window': LAMEHIP_MID_WINDOW is set by the
parent, and the encode launches must have run in windows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    mode = sys.argv[1]
    torch.zeros(1, device="cuda:0")
    import lamehip
    import pcm_input_support as psup
    import test_append_input_device as ta
    import test_pcm_input_device as t
    stype, sr, out, kw, B, step = lamehip.PCM_F32_UNIT, 48000, 44100, dict(brate=128), 4, 1152
    lens = [int(0.4 * sr) + 531 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9950 + s, lens[s], sr) for s in range(B)]
    cap = max(lens) + 2
    host = np.full((B, 2, cap), np.nan, np.float32)
    for s, x in enumerate(xs):
        host[s, :, :lens[s]] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    enc = t.open_product(sr, kw, out)
    whole = lamehip.Batch(enc, B, cap)
    whole.set_device_resampling()
    whole.set_sample_type(stype)
    t.feed(whole, xs, False, False)
    whole.encode()
    want = [whole.pack(s) for s in range(B)]
    floats = [whole.converted(s) for s in range(B)]
    whole.close()
    b = lamehip.Batch(enc, B, cap)
    b.set_device_resampling()
    b.set_sample_type(stype)
    b.set_incremental_resampling()
    got = [b""] * B
    # (appends per stream between two encode_available: five frames' worth, so that a launch has more than one window)
    per_round = 5 if mode == "window" else 1
    pos, rnd, windows, ms = [0] * B, 0, [], 0.0
    while any(pos[s] < lens[s] for s in range(B)):
        ns = [min(step, lens[s] - pos[s]) for s in range(B)]
        how = rnd % 4
        from_host = [(s + rnd // 4) % 2 == 1 for s in range(B)]        # one stream of each pair, the other one next time
        if how < 3:
            in_tensor = [0 if from_host[s] else ns[s] for s in range(B)]
            T = step + 5
            big = torch.full((B, 2, T + 9), float("nan"), device="cuda:0")
            chunk = big[:, :, 3:3 + T] if how == 1 else torch.full((B, 2, T), float("nan"), device="cuda:0")
            for s in range(B):
                chunk[s, :, :in_tensor[s]] = dev[s, :, pos[s]:pos[s] + in_tensor[s]]
            if how == 2:
                chunk = chunk.permute(0, 2, 1).contiguous()             # [B, T, 2]
            torch.cuda.synchronize()                                    # the producer has finished
            for s in range(B):
                if from_host[s] and s % 2 == 0:                         # (staged before the device round, or behind it)
                    b.append_input(s, xs[s][0, pos[s]:pos[s] + ns[s]], xs[s][1, pos[s]:pos[s] + ns[s]])
            b.append_device(chunk, in_tensor)
            for s in range(B):
                if from_host[s] and s % 2 == 1:
                    b.append_input(s, interleaved=np.ascontiguousarray(xs[s][:, pos[s]:pos[s] + ns[s]].T))
            chunk.fill_(float("nan"))                                   # reusable at once
        else:
            for s in range(B):
                a, e = pos[s], pos[s] + ns[s]
                if from_host[s]:
                    b.append_input(s, xs[s][0, a:e], xs[s][1, a:e])
                elif s < 2:
                    b.append_input(s, dev[s, 0, a:e], dev[s, 1, a:e])
                else:
                    pairs = dev[s, :, a:e].t().contiguous()             # [n, 2]
                    torch.cuda.synchronize()
                    b.append_input(s, interleaved=pairs)
        for s in range(B):
            pos[s] += ns[s]
        rnd += 1
        if rnd % per_round:
            continue
        b.encode_available()
        windows.append(b.windows())
        ms += b.resample_ms()
        ta.drain_all(b, got)
    b.finish()
    windows.append(b.windows())
    ta.drain_all(b, got)
    for s in range(B):
        assert got[s] == want[s], s
        assert psup.same_floats(b.converted(s), floats[s]), s
    assert rnd > 8 and ms > 0.0
    if mode == "window":
        assert os.environ.get("LAMEHIP_MID_WINDOW") == "3" and max(windows) > 1, windows
    else:
        assert max(windows) == 1, windows
    b.close()
    enc.close()
    print("incremental conversion ok: %s, %d rounds, windows %r" % (mode, rnd, sorted(set(windows))), flush=True)


if __name__ == "__main__":
    main()
