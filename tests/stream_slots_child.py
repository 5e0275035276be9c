"""Child process of tests/test_stream_slots_device.py::test_everything_on_top_fed_from_a_tensor: torch takes the device first,
then ten float32 utterances at +/- 1.0 -- held as one tensor on the same GPU, NaN beyond each length -- come and go over four
slots of an incremental batch that converts 48 -> 44.1 kHz, measures ReplayGain, packs on the device and carries tag frames,
all round by round, fed through append_device in ragged chunks (also of 0 and 1 samples).  For every utterance the bytes, the
tag with the gain in it, the radio gain and the gain windows are those of a fresh ONE-stream incremental batch with the same
switches, fed the same appends and ended by finish(): a path that knows nothing of the slot calls."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def full_batch(lamehip, enc, stype, B, cap):
    b = lamehip.Batch(enc, B, cap)
    b.set_device_resampling()
    b.set_sample_type(stype)
    b.set_device_packing()
    b.set_incremental_packing()
    b.set_incremental_resampling()
    b.set_incremental_replaygain()
    b.set_incremental_tagging()
    return b


def main():
    torch.zeros(1, device="cuda:0")
    import lamehip
    import pcm_input_support as psup
    import stream_slots_support as ss
    import test_pcm_input_device as t
    stype, sr, out, kw, B, N = lamehip.PCM_F32_UNIT, 48000, 44100, dict(brate=128), 4, 10
    rng = np.random.default_rng(7300)
    lens = [int(sr * rng.uniform(0.3, 0.6)) | 1 for _ in range(N)]
    xs = [psup.typed_signal(stype, 7310 + u, lens[u], sr) for u in range(N)]
    cap = max(lens) + 2
    host = np.full((N, 2, cap), np.nan, np.float32)
    for u, x in enumerate(xs):
        host[u, :, :lens[u]] = x
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    rounds = ss.schedule(np.random.default_rng(7301), lens, B)
    enc = t.open_product(sr, kw, out)
    # the references: every utterance alone, the same appends (the chunks of its rounds), finish
    want = {}
    for u in range(N):
        one = full_batch(lamehip, enc, stype, 1, cap)
        got = b""
        for appends, ends, restarts in rounds:
            for s, uu, a, e in appends:
                if uu != u:
                    continue
                chunk = torch.full((1, 2, e - a + 5), float("nan"), device="cuda:0")
                chunk[0, :, :e - a] = dev[u, :, a:e]
                torch.cuda.synchronize()
                one.append_device(chunk, [e - a])
                one.encode_available()
                got += one.drain(0)
        one.finish()
        got += one.drain(0)
        want[u] = (got, one.tag(0), one.radio_gain(0), one.gain_windows(0).tobytes(), one.frames(0))
        one.close()
    b = full_batch(lamehip, enc, stype, B, cap)
    T = b.tag_size()
    assert T > 0
    got, ms, nrestart = {u: b"" for u in range(N)}, 0.0, 0
    for appends, ends, restarts in rounds:
        ns = [0] * B
        for s, u, a, e in appends:
            ns[s] = e - a
        chunk = torch.full((B, 2, max(ns) + 5), float("nan"), device="cuda:0")
        for s, u, a, e in appends:
            chunk[s, :, :e - a] = dev[u, :, a:e]
        torch.cuda.synchronize()                                        # the producer has finished
        b.append_device(chunk, ns)
        for s in ends:
            b.end_stream(s)
        b.encode_available()
        ms += b.restart_ms()
        for s, u, a, e in appends:
            got[u] += b.drain(s)
            assert b.stream_ended(s) is (s in ends)
        for s, u, nxt in restarts:
            have = (got[u], b.tag(s), b.radio_gain(s), b.gain_windows(s).tobytes(), b.frames(s))
            for k, what in enumerate(("bytes", "tag", "radio gain", "gain windows", "frames")):
                assert have[k] == want[u][k], "utterance %d: %s" % (u, what)
            assert b.tag(s) == want[u][1]                               # (handed out twice: patched once)
            b.restart_stream(s)
            nrestart += 1
    assert nrestart == N and ms > 0.0 and len(rounds) > 5
    b.close()
    enc.close()
    print("stream slots ok: %d utterances over %d slots in %d rounds, %d bytes of tags" % (N, B, len(rounds), N * T), flush=True)


if __name__ == "__main__":
    main()
