"""Child process of tests/test_append_replaygain_device.py::test_mapping_forced_and_a_round_from_torch, started with
LAMEHIP_GAIN_LANES=0 or 1: torch takes the device first, then the ragged s16 batch of the first setting goes through an
incremental batch that measures ReplayGain round by round -- one of its rounds through append_device from an int16 [B, 2, T]
tensor on the same GPU, one call per stream, the others from host and device arrays as in the parent's tests.  After every
round the windows are the host twin's, after finish the gains are the handle's fed the same calls."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    assert os.environ.get("LAMEHIP_GAIN_LANES") in ("0", "1")
    torch.zeros(1, device="cuda:0")
    import append_replaygain_support as sup
    import gain_support as gs
    import test_append_replaygain_device as t
    setting, K = gs.SETTINGS[0], 2
    xs = [gs.signal(setting, 9500 + s, n, 1.0 if s % 2 == 0 else 0.25) for s, n in enumerate(t.lengths_of(setting))]
    rounds = [sup.into_rounds(sup.calls_of(setting, s, x.shape[1]), 11 + s) for s, x in enumerate(xs)]
    for r in rounds:                    # round K: one call per stream, the tensor's
        if K < len(r):
            r[K] = [sum(r[K])] if sum(r[K]) > 0 else []
    gains = [sup.handle_calls(setting, x, [m for k in r for m in k])[1] for x, r in zip(xs, rounds)]

    def from_tensor(b, xs, pos, ns):
        T = max(ns) + 5
        host = np.full((len(xs), 2, T), 0x7fff, np.int16)
        for s, x in enumerate(xs):
            host[s, :, :ns[s]] = x[:, pos[s]:pos[s] + ns[s]]
        chunk = torch.from_numpy(host).to("cuda:0")
        torch.cuda.synchronize()        # the producer has finished
        b.append_device(chunk, ns)
        chunk.fill_(0x7fff)             # reusable at once
        return ns

    got, wins, ms = t.run_rounds(setting, xs, rounds, gains=gains, torch_round=(K, from_tensor),
                                 what="LAMEHIP_GAIN_LANES=%s," % os.environ["LAMEHIP_GAIN_LANES"])
    assert ms > 0.0 and sum(len(w) for w in wins) > 30 and max(sum(r[K]) for r in rounds if K < len(r)) > 0
    print("incremental gain ok: lanes %s, %d windows" % (os.environ["LAMEHIP_GAIN_LANES"], sum(len(w) for w in wins)), flush=True)


if __name__ == "__main__":
    main()
