"""GPU: CBR / ABR launches of the split pipeline behind the front masking kernels (csrc/lh_psy_finish.hip) -- every frame of
every stream against the oracle, every stream's packed bytes against the host packer over the oracle's frames; the state
hand-over to and from every other kind of launch; the VBR loops on their untouched path; and, through the dump library, a
census that the CBR / ABR launches really started from the LhMidPsy records.  Small batches: 2 - 4 streams of 2 - 3 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import lamehip
from lamehip.types import struct_diff

pytestmark = pytest.mark.gpu

DUMP_LIB = os.path.join(helpers.ROOT, "deprecated-lame-mirror_amd", "lamehip", "liblamehip_dump.so")


def _signal(kind, seed, n, sr):
    if kind == "silence":
        # 2.5 s of digital silence pull the ATH factor down to its floor (0.925 a frame: below 0.000625 after ~95 frames),
        # the burst swings it back, and the clamp meets previous calls that left nothing
        rng = np.random.Generator(np.random.PCG64(seed))
        n0 = int(2.5 * sr)
        x = np.zeros((2, n))
        x[:, n0:] = 20000 * rng.standard_normal((2, n - n0)) * np.exp(-np.arange(n - n0) / 2500.0)
        return x.clip(-32768, 32767).astype(np.int16)
    return helpers.synth_stream(seed, n, sr, burst_interval=1.0 / kind)


def _batch(enc, pcms, mono=False):
    b = lamehip.Batch(enc, len(pcms), max(x.shape[1] for x in pcms) + 16)
    for s, x in enumerate(pcms):
        if mono:
            b.set_pcm(s, x[0])
        else:
            b.set_pcm(s, x[0], x[1])
    return b


def _check(enc, b, pcms, orc, what):
    cfg, tab = enc.config(), enc.tables()
    for s, x in enumerate(pcms):
        got, want = b.get_frames(s), orc.encode_frames(cfg, tab, x)
        assert len(got) == len(want), (what, s)
        for f in range(len(want)):
            d = struct_diff(want[f], got[f])
            assert not d, (what, s, f, d[:4])
        assert b.pack(s) == helpers.pack_frames(enc.lib, cfg, tab, want), (what, s)


# (id, settings, signal: bursts per second or "silence", stream lengths in samples)
CASES = [
    ("cbr128_js_b3", dict(brate=128), 3, (88200, 100001, 70000)),
    # 40 bursts a second: short, start and stop blocks in both channels, attacks in consecutive granules, last_attacks == 3;
    # with a stream of two frames, whose launch takes the clamp's previous calls from the state alone
    ("cbr128_js_b40", dict(brate=128), 40, (88200, 1000, 99999, 132300)),
    ("cbr128_stereo", dict(brate=128, mode=0), 40, (88200, 77777)),
    ("cbr128_mono", dict(brate=128, channels=1), 40, (88200, 77777)),
    ("abr128_js", dict(abr=128), 40, (88200, 100001, 60000)),
    ("cbr320_48k_b40", dict(samplerate=48000, brate=320), 40, (96000, 120001)),
    ("cbr128_silence_burst", dict(brate=128), "silence", (132300, 140000)),
]


@pytest.mark.parametrize("name,kw,signal,lens", CASES, ids=[c[0] for c in CASES])
def test_front_launch_matches_oracle(name, kw, signal, lens, oracle):
    kw = dict(kw)
    sr = kw.pop("samplerate", 44100)
    mono = kw.get("channels", 2) == 1
    enc = lamehip.Encoder(sr, **kw)
    pcms = [_signal(signal, 700 + 10 * s, n, sr) for s, n in enumerate(lens)]
    if mono:
        pcms = [np.stack([x[0], x[0]]) for x in pcms]
    b = _batch(enc, pcms, mono)
    b.encode()
    split, parts = b.kernel_parts_ms()
    assert split and b.windows() == 1 and all(p > 0 for p in parts)
    if name == "cbr128_js_b40":
        assert b.frames(1) == 2
    _check(enc, b, pcms, oracle, name)
    b.close()
    enc.close()


@pytest.mark.parametrize("kw", [dict(vbr_q=2), dict(vbr_q=2, vbr_mode=2)], ids=["vbr2", "vbrold2"])
def test_vbr_launches_keep_their_path(kw, oracle):
    """The VBR loops feed the perceptual entropy back into the masking adjustment: no front kernels, same payload."""
    sr = 44100
    enc = lamehip.Encoder(sr, **kw)
    pcms = [helpers.synth_stream(900 + s, 88200 + 1000 * s, sr, burst_interval=1.0 / 40) for s in range(2)]
    b = _batch(enc, pcms)
    b.encode()
    assert b.kernel_parts_ms()[0]
    _check(enc, b, pcms, oracle, str(kw))
    b.close()
    enc.close()


@pytest.mark.parametrize("how", ["two_launches", "rounds_1s", "windows_3", "split_deny"])
def test_hand_over_equals_one_shot(how, monkeypatch):
    """The same PCM through an incremental batch -- in two launches, in rounds of 1 s, with every launch in windows of three
    frames (LAMEHIP_MID_WINDOW=3), with fused and split launches taking turns (LAMEHIP_SPLIT_DENY) -- gives the one-shot
    batch's bytes: a launch behind the front kernels leaves and finds LhStreamState as every other launch does."""
    sr, B = 44100, 3
    enc = lamehip.Encoder(sr, 128)
    lens = [3 * sr + 977 * s for s in range(B)]
    pcms = [helpers.synth_stream(1300 + s, lens[s], sr, burst_interval=1.0 / 40) for s in range(B)]
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "0")
    monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "0")
    one = _batch(enc, pcms)
    one.encode()
    assert one.kernel_parts_ms()[0] and one.windows() == 1
    want = [one.pack(s) for s in range(B)]
    one.close()
    if how == "windows_3":
        # (a one-shot launch in windows)
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", "3")
        b = _batch(enc, pcms)
        b.encode()
        assert b.windows() > 1 and b.kernel_parts_ms()[0]
        assert [b.pack(s) for s in range(B)] == want
        b.close()
    step = {"two_launches": 2 * sr, "rounds_1s": sr, "windows_3": sr, "split_deny": sr // 2}[how]
    b = lamehip.Batch(enc, B, max(lens) + 16)
    got = [b""] * B
    pos, rnd, kinds = 0, 0, []
    while pos < max(lens):
        for s in range(B):
            a, e = min(pos, lens[s]), min(pos + step, lens[s])
            if e > a:
                b.append(s, np.ascontiguousarray(pcms[s][0][a:e]), np.ascontiguousarray(pcms[s][1][a:e]))
        if how == "split_deny":
            monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "1" if rnd % 2 else "0")
        b.encode_available()
        kinds.append(bool(b.kernel_parts_ms()[0]))
        for s in range(B):
            got[s] += b.drain(s)
        pos += step
        rnd += 1
    monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "0")
    b.finish()
    for s in range(B):
        got[s] += b.drain(s)
        assert got[s] == want[s], (how, s)
    if how == "split_deny":
        assert True in kinds and False in kinds, kinds
    else:
        assert all(kinds), kinds
    b.close()
    enc.close()


def test_census_cbr_launches_start_from_the_front_records():
    """Dump library, one child process (tests/psy_finish_census_child.py): every frame of a CBR and of an ABR batch counted
    a prologue that started from an LhMidPsy record, no frame of a VBR batch did, a fused launch (LAMEHIP_SPLIT_DENY) counts
    none -- so a silent fall-back to the old prologue fails here --, and the last frame's band energies / thresholds,
    perceptual entropies and bit budgets (dbg_en, dbg_thm, dbg_pe, dbg_targ) are the committed stage fixture's, 0 ulp."""
    assert os.path.exists(DUMP_LIB), "make -C deprecated-lame-mirror_amd/csrc dump"
    env = dict(os.environ, LAMEHIP_LIB=DUMP_LIB)
    for k in ("LAMEHIP_FUSED", "LAMEHIP_SPLIT_DENY", "LAMEHIP_MID_WINDOW"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "tests", "psy_finish_census_child.py")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("CENSUS ")]
    assert line, out.stdout[-2000:]
    res = json.loads(line[0][7:])
    for what in ("cbr128", "abr128"):
        assert res[what]["frames"] > 60 and res[what]["front"] == res[what]["frames"], res
    assert res["vbr2"]["frames"] > 60 and res["vbr2"]["front"] == 0, res
    assert res["cbr128_fused"]["frames"] > 60 and res["cbr128_fused"]["front"] == 0, res
    assert res["fixture_frames"] >= 3 and res["fixture_bad"] == [], res
