"""Child process of tests/test_psy_finish_device.py::test_census_cbr_launches_start_from_the_front_records, started with
LAMEHIP_LIB naming the dump library (liblamehip_dump.so, -DLH_DEBUG_DUMP: the binding loads one library per process).  The
dump build counts, per stream, the frames whose prologue started from an LhMidPsy record (LhStreamState.dbg_front_frames, the
third word from the end of the state) and keeps what the stages of a launch's last frame handed on.  Prints one line:
CENSUS {json}."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import helpers  # noqa: E402
import lamehip  # noqa: E402

TAIL_FLOATS = 2 * 2 * 576 + 2 * 2 * 40 + 2 * (2 * 2 * 64) + 4 + 4 + 1 + 3      # (tests/test_stage_fixtures.py)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def state_tail(enc, b, s):
    size = enc.lib.lamehip_abi_sizeof(4)
    buf = C.create_string_buffer(size)
    assert enc.lib.lamehip_batch_get_state(b.b, s, buf, size) == size
    return np.frombuffer(buf.raw[size - 4 * TAIL_FLOATS:], dtype=np.float32)


def front_frames(enc, b, s):
    return int(state_tail(enc, b, s).view(np.int32)[-3])


def main():
    assert os.environ.get("LAMEHIP_LIB", "").endswith("liblamehip_dump.so")
    res = {}
    sr = 44100
    pcms = [helpers.synth_stream(2100 + s, 2 * sr + 500 * s, sr, burst_interval=1.0 / 40) for s in range(2)]
    for what, kw, deny in (("cbr128", dict(brate=128), "0"), ("abr128", dict(abr=128), "0"), ("vbr2", dict(vbr_q=2), "0"),
                           ("cbr128_fused", dict(brate=128), "1")):
        os.environ["LAMEHIP_SPLIT_DENY"] = deny
        enc = lamehip.Encoder(sr, **kw)
        b = lamehip.Batch(enc, len(pcms), max(x.shape[1] for x in pcms) + 16)
        for s, x in enumerate(pcms):
            b.set_pcm(s, x[0], x[1])
        b.encode()
        assert bool(b.kernel_parts_ms()[0]) == (deny == "0"), what
        res[what] = {"frames": sum(b.frames(s) for s in range(len(pcms))),
                     "front": sum(front_frames(enc, b, s) for s in range(len(pcms)))}
        b.close()
        enc.close()
    os.environ["LAMEHIP_SPLIT_DENY"] = "0"
    # the committed stage fixture (tests/golden/stages_cbr128_js_44k.npz: hashes of the reference's values per frame): the
    # golden stream in rounds of ten frames, the last frame of every launch observed
    name = "cbr128_js_44k"
    z = np.load(os.path.join(helpers.ROOT, "tests", "golden", "stages_%s.npz" % name))
    g, pcm = helpers.load_golden(name)
    enc = lamehip.Encoder(require_device=True, **helpers.golden_encoder_kwargs(g))
    n = pcm.shape[1]
    b = lamehip.Batch(enc, 1, n + 4608)
    done, seen, bad = 0, 0, []
    for i in range(0, n, 11520):
        b.append(0, np.ascontiguousarray(pcm[0][i:i + 11520]), np.ascontiguousarray(pcm[1][i:i + 11520]))
        k = b.encode_available()
        b.sync()
        if k <= 0:
            continue
        done += k
        assert b.kernel_parts_ms()[0]
        t = state_tail(enc, b, 0)
        assert int(t.view(np.int32)[-3]) == done, "a launch of the fixture stream did not start from the front records"
        o = 2304 + 160
        en = t[o:o + 256].reshape(2, 2, 64)[:, :, :61]
        thm = t[o + 256:o + 512].reshape(2, 2, 64)[:, :, :61]
        pe = t[o + 512:o + 516]
        targ = t[o + 516:o + 521].view(np.int32)
        f = done - 1
        for key, val in (("en", en), ("thm", thm), ("pe", pe), ("targ", targ)):
            if sha(val) != str(z[key][f]):
                bad.append([f, key])
        seen += 1
    res["fixture_frames"] = seen
    res["fixture_bad"] = bad
    b.close()
    enc.close()
    print("CENSUS " + json.dumps(res))


if __name__ == "__main__":
    main()
