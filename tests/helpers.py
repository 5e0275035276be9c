"""Shared test helpers: seeded synthetic PCM (SURVEY.md 8(d) recipe), loaders for
the CPU oracle and -- when it was built in this tree -- the compiled reference."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deprecated-lame-mirror_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from lamehip.types import (LhConfig, LhFrameOut, LhInitAux, LhTables, LhUserParams)  # noqa: E402

ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle.so")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")


def synth_stream(seed, n, sr=44100, burst_interval=None, white=False):
    """Music-like seeded stereo s16: 8 partials with independent channel phases,
    low-level brown noise, decaying white-noise bursts (castanet-like -> short
    blocks).  burst_interval in seconds (default 1/3)."""
    rng = np.random.Generator(np.random.PCG64(0x4C414D45 + seed))
    if white:
        return (rng.standard_normal((2, n)) * 8000).clip(-32768, 32767).astype(np.int16)
    t = np.arange(n) / sr
    x = np.zeros((2, n))
    for k in range(8):
        f = 220.0 * 2 ** (k / 2.0)
        vib = 1.0 + 0.001 * np.sin(2 * np.pi * 5 * t)
        for c in range(2):
            x[c] += 0.5 / (k + 1) * np.sin(2 * np.pi * f * t * vib + rng.uniform(0, 2 * np.pi))
    brown = np.cumsum(rng.standard_normal((2, n)), axis=1)
    k = 200
    cs = np.cumsum(np.pad(brown, ((0, 0), (k, 0)), mode="edge"), axis=1)
    brown = brown - (cs[:, k:] - cs[:, :-k]) / k
    x += 0.02 * brown / (np.abs(brown).max() + 1e-9)
    step = int(sr * (burst_interval if burst_interval else 1.0 / 3))
    for s in range(step // 2, n, max(step, 1)):
        m = min(2000, n - s)
        env = np.exp(-np.arange(m) / 300.0)
        x[:, s:s + m] += 0.6 * env * rng.standard_normal((2, m))
    x = x / np.abs(x).max() * 0.8 * 32767
    return x.astype(np.int16)


def locked_make(args, cwd):
    """make under a file lock: pytest-xdist workers that find the same target stale would otherwise build it at once"""
    import fcntl
    with open(os.path.join(cwd, ".make.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            subprocess.check_call(["make"] + list(args), cwd=cwd, stdout=subprocess.DEVNULL)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def build_oracle():
    if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < max(
            os.path.getmtime(os.path.join(ROOT, "oracle", f)) for f in os.listdir(os.path.join(ROOT, "oracle"))
            if f.endswith((".c", ".h"))):
        locked_make(["oracle"], os.path.join(ROOT, "oracle"))
    return ORACLE_SO


class Oracle:
    """CPU restatement (oracle/lame_oracle.c) -- the checker, never the product."""

    def __init__(self):
        self.lib = C.CDLL(build_oracle())

    def encode_frames(self, cfg, tab, pcm, max_frames=None):
        left = np.ascontiguousarray(pcm[0], dtype=np.int16)
        right = np.ascontiguousarray(pcm[1], dtype=np.int16)
        n = len(left)
        nf = self.lib.orc_total_frames_fs(C.c_long(n), 576 * cfg.mode_gr)
        if max_frames is not None:
            nf = min(nf, max_frames)
        out = (LhFrameOut * nf)()
        self.lib.orc_encode_stream(C.byref(cfg), C.byref(tab), left.ctypes.data_as(C.c_void_p),
                                   right.ctypes.data_as(C.c_void_p), C.c_long(n), out, nf, None)
        return out

    def encode_frames_census(self, cfg, tab, pcm):
        """encode_frames plus what tests/test_route_census.py predicts routes from: the spectra as the quantiser left them
        in place, float32 [frame][gr][ch][576] (after the mid/side rotation, the short-block reordering and, under the old
        VBR loop, the analog-silence edit of the top band), and the loops' pass counters for this stream."""
        left = np.ascontiguousarray(pcm[0], dtype=np.int16)
        right = np.ascontiguousarray(pcm[1], dtype=np.int16)
        n = len(left)
        nf = self.lib.orc_total_frames_fs(C.c_long(n), 576 * cfg.mode_gr)
        out = (LhFrameOut * nf)()
        xr = np.zeros((nf, 2, 2, 576), np.float32)
        names = ("orc_old_pass_frames", "orc_old_pass_extra", "orc_vbr_pass2_frames")
        for k in names:
            C.c_int.in_dll(self.lib, k).value = 0
        self.lib.orc_encode_stream(C.byref(cfg), C.byref(tab), left.ctypes.data_as(C.c_void_p),
                                   right.ctypes.data_as(C.c_void_p), C.c_long(n), out, nf, xr.ctypes.data_as(C.c_void_p))
        return out, xr, {k: C.c_int.in_dll(self.lib, k).value for k in names}


class Reference:
    """The real reference encoder built by oracle/Makefile (only in trees where
    /root/reference existed at build time)."""

    def __init__(self):
        if not os.path.exists(REF_SO):
            raise FileNotFoundError(REF_SO)
        self.lib = C.CDLL(REF_SO)
        self.lib.refh_open.restype = C.c_void_p
        self.lib.refh_open_vbr.restype = C.c_void_p
        self.lib.refh_open_abr.restype = C.c_void_p
        self.lib.refh_encode_stream.restype = C.c_long

    def encode(self, pcm, sr, brate, mode=-1, quality=-1, max_frames=0, vbr_q=None, out_samplerate=0, abr=None,
               channels=2, vbr_mode=4):
        """CBR at `brate', VBR (vbr_mode: 4 vbr_mtrh, 1 vbr_mt, 2 vbr_rh) at quality vbr_q, or ABR at a mean of
        `abr' kb/s; channels=1: mono (only pcm[0] is read)."""
        self.lib.refh_set_channels(channels)
        self.lib.refh_set_vbr_mode(vbr_mode)
        left = np.ascontiguousarray(pcm[0], dtype=np.int16)
        right = np.ascontiguousarray(pcm[1], dtype=np.int16)
        n = len(left)
        if abr is not None:
            h = self.lib.refh_open_abr(sr, abr, mode, quality, out_samplerate, 0)
        elif vbr_q is None:
            h = self.lib.refh_open(sr, brate, mode, quality)
        else:
            h = self.lib.refh_open_vbr(sr, vbr_q, mode, quality, out_samplerate, 0)
        self.lib.refh_set_vbr_mode(4)       # (a setting of the harness, not of the handle: back to the default)
        assert h, "reference refused the settings"
        h = C.c_void_p(h)
        buf = C.create_string_buffer(2 * n + 100000)
        nf = C.c_int(0)
        frames = (LhFrameOut * max(max_frames, 1))()
        k = self.lib.refh_encode_stream(h, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p),
                                        C.c_long(n), buf, C.c_long(len(buf)), frames if max_frames else None,
                                        None, max_frames, C.byref(nf))
        cfg, tab = LhConfig(), LhTables()
        self.lib.refh_get_config(h, C.byref(cfg))
        self.lib.refh_get_tables(h, C.byref(tab))
        self.lib.refh_close(h)
        assert k >= 0
        return buf.raw[:k], nf.value, frames, cfg, tab


def reference_tagged(pcm, sr, brate, mode=-1, quality=-1, chunk=1152, vbr_q=None, abr=None, channels=2, vbr_mode=4):
    """The compiled reference with its default tag handling (bWriteVbrTag = 1): returns
    (stream bytes incl. the placeholder frame, final tag frame).  vbr_q selects VBR (vbr_mode as in Reference.encode)."""
    ref = Reference()
    lib = ref.lib
    lib.refh_open_tag.restype = C.c_void_p
    lib.refh_set_channels(channels)
    lib.refh_set_vbr_mode(vbr_mode)
    if abr is not None:
        h = lib.refh_open_abr(sr, abr, mode, quality, 0, 1)
    elif vbr_q is None:
        h = lib.refh_open_tag(sr, brate, mode, quality)
    else:
        h = lib.refh_open_vbr(sr, vbr_q, mode, quality, sr if vbr_q >= 7 else 0, 1)
    lib.refh_set_vbr_mode(4)
    assert h, "reference refused the settings"
    h = C.c_void_p(h)
    left = np.ascontiguousarray(pcm[0], dtype=np.int16)
    right = np.ascontiguousarray(pcm[1], dtype=np.int16)
    n = len(left)
    buf = C.create_string_buffer(int(1.25 * chunk) + 7200 + 3000)
    out = b""
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        k = lib.refh_encode(h, left[i:].ctypes.data_as(C.c_void_p), right[i:].ctypes.data_as(C.c_void_p), m,
                            buf, len(buf))
        assert k >= 0
        out += buf.raw[:k]
    k = lib.refh_flush(h, buf, len(buf))
    assert k >= 0
    out += buf.raw[:k]
    t = C.create_string_buffer(2880)
    k = lib.refh_lametag(h, t, len(t))
    tag = t.raw[:k]
    lib.refh_close(h)
    return out, tag


def have_reference():
    return os.path.exists(REF_SO)


def normalize_tables(frames):
    """Table 14 is an estimate-only code book; the packer (like the reference's
    encodeSideInfo2) writes 16 in its place.  Frames captured from the reference
    after format_bitstream already carry 16."""
    for fr in frames:
        for g in fr.gr:
            for gg in g:
                for k in range(3):
                    if gg.table_select[k] == 14:
                        gg.table_select[k] = 16
    return frames


GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def golden_names(vbr=False, kind=None):
    """Fixtures by kind: stereo CBR by default, vbr=True / kind="vbr" the vbr_mtrh ones, kind="abr"
    the ABR ones, kind="mono" the one-channel ones of any rate control (the kind is in the file name)."""
    kind = kind or ("vbr" if vbr else "cbr")

    def k(f):
        return "mono" if f.startswith("mono_") else "vbr" if "vbr" in f else ("abr" if "abr" in f else "cbr")
    # (stages_*.npz are the per-stage fixtures of tests/test_stage_fixtures.py, not whole-stream goldens)
    return sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.endswith(".npz") and not f.startswith("stages_") and k(f) == kind)


def load_golden(name):
    """Returns (dict of fixture fields, pcm int16 [2, n]) -- the input is rebuilt
    from its committed recipe (or read from the reference's own testcase.wav)."""
    import wave
    g = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False))
    seed, secs, burst, white = g["recipe"]
    sr = int(g["samplerate"])
    if seed == -2:
        w = wave.open(os.path.join(GOLDEN_DIR, "testcase.wav"))
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).reshape(-1, 2).T
    elif seed < 0:
        pcm = np.zeros((2, int(g["nsamples"])), np.int16)
    else:
        pcm = synth_stream(int(seed), int(sr * secs), sr, burst if burst > 0 else None, bool(white))
    if "channels" in g and int(g["channels"]) == 1:
        pcm = np.stack([pcm[0], pcm[0]])
    assert pcm.shape[1] == int(g["nsamples"])
    return g, np.ascontiguousarray(pcm)


def golden_settings(g):
    mode = int(g["mode"])
    q = int(g["quality"])
    return int(g["samplerate"]), int(g["brate"]), (None if mode < 0 else mode), (None if q < 0 else q)


def golden_vbr_q(g):
    """None for a CBR fixture, else the vbr_mtrh quality (-V n) it was made with."""
    v = int(g["vbr_q"]) if "vbr_q" in g else -1
    return None if v < 0 else v


def golden_encoder_kwargs(g):
    """Keyword arguments of lamehip.Encoder for a fixture of any kind."""
    sr, br, mode, q = golden_settings(g)
    return dict(samplerate=sr, brate=br, mode=mode, quality=q, vbr_q=golden_vbr_q(g), abr=golden_abr(g),
                channels=int(g["channels"]) if "channels" in g else 2,
                vbr_mode=int(g["vbr_mode"]) if "vbr_mode" in g else 4)


def golden_abr(g):
    """None, or the mean bitrate of an ABR fixture."""
    v = int(g["abr"]) if "abr" in g else -1
    return None if v < 0 else v


def frame_sha(fr):
    import hashlib
    return hashlib.sha256(bytes(fr)).hexdigest()


def pack_frames(lib, cfg, tab, frames):
    """Run the PRODUCT's host bit packer (lh_bitstream.c inside liblamehip.so) over a
    list of LhFrameOut; returns the byte stream."""
    bs = C.create_string_buffer(64 * 1024)
    assert lib.lh_bs_init(bs) == 0
    out = b""
    tmp = C.create_string_buffer(32768)
    for fr in frames:
        rc = lib.lh_bs_format_frame(bs, C.byref(cfg), C.byref(tab), C.byref(fr))
        assert rc == 0, "packer consistency check %d" % rc
        k = lib.lh_bs_copy(bs, tmp, len(tmp))
        out += tmp.raw[:k]
    lib.lh_bs_flush(bs, C.byref(cfg), C.byref(frames[len(frames) - 1]) if len(frames) else None)
    k = lib.lh_bs_copy(bs, tmp, len(tmp))
    out += tmp.raw[:k]
    lib.lh_bs_free(bs)
    return out
