"""Rate conversion of a batch on the device (lamehip_batch_set_device_resampling, csrc/lh_resample_dev.hip): the floats
the encoder reads are the host conversion's bit for bit, so the bytes are those of the same batch converting on the host
(and the reference's); device-resident input, the pinned mirror and the pipelined calls work on such a batch."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import lamehip
import resample_support as rsup
from test_resample import CASES, IDS, open_product, open_reference, reference_calls

pytestmark = pytest.mark.gpu


def case_lengths(rate_in):
    return [int(rate_in * 1.2), 5000, 1, 0, 1151, 1152, 1153, int(rate_in * 0.5) + 13]


def fill(b, pcms):
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])


@functools.lru_cache(maxsize=None)
def case_data(case):
    """per entry of CASES, computed once: the streams, and what a batch that converts on the host makes of them --
    converted floats (its own and the pure host function's), host-packed and device-packed bytes"""
    rate_in, kw, out, rate_out = CASES[case]
    lens = case_lengths(rate_in)
    pcms = [helpers.synth_stream(7500 + 10 * case + i, n, rate_in, 1.0 / 9) if n else np.zeros((2, 0), np.int16)
            for i, n in enumerate(lens)]
    enc = open_product(rate_in, kw, out, require_device=True)
    cfg = enc.config()
    b = lamehip.Batch(enc, len(pcms), max(lens))
    b.set_device_packing()
    fill(b, pcms)
    b.encode()
    lib = rsup.library()
    floats = []
    for s, x in enumerate(pcms):
        want = rsup.host_convert(lib, rate_in, rate_out, cfg.channels, cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r, x)[0]
        assert rsup.same_floats(b.converted(s), want), "host path, stream %d" % s
        floats.append(want)
    packed = [b.pack(s) for s in range(len(pcms))]
    for s in range(len(pcms)):
        assert b.get_bytes(s) == packed[s]
    frames = [b.frames(s) for s in range(len(pcms))]
    assert b.resample_ms() == 0.0
    b.close()
    enc.close()
    return pcms, floats, packed, frames


def device_batch(enc, pcms, cap=None):
    b = lamehip.Batch(enc, len(pcms), cap or max(x.shape[1] for x in pcms))
    b.set_device_packing()
    b.set_device_resampling()
    return b


def check_bytes(b, packed, what=""):
    for s, want in enumerate(packed):
        assert b.pack(s) == want, "%s stream %d (host packer)" % (what, s)
        assert b.get_bytes(s) == want, "%s stream %d (device packer)" % (what, s)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_device_conversion_equals_host_conversion(case):
    """every rate case, both packers: floats == host conversion, bytes == the batch converting on the host, and -- where
    the compiled reference is present -- == the reference fed 1152 samples per call"""
    rate_in, kw, out, rate_out = CASES[case]
    pcms, floats, packed, frames = case_data(case)
    enc = open_product(rate_in, kw, out, require_device=True)
    b = device_batch(enc, pcms)
    fill(b, pcms)
    assert [b.frames(s) for s in range(len(pcms))] == frames        # known from the plan, before anything ran
    b.encode()
    assert b.resample_ms() > 0.0
    for s, want in enumerate(floats):
        assert rsup.same_floats(b.converted(s), want), "stream %d" % s
    check_bytes(b, packed)
    if helpers.have_reference():
        ref = helpers.Reference()
        for s, x in enumerate(pcms):
            h = open_reference(ref, rate_in, kw, out)
            calls, tail = reference_calls(ref, h, x, [1152])
            ref.lib.refh_close(h)
            assert packed[s] == b"".join(c[2] for c in calls) + tail, "stream %d (reference)" % s
    b.close()
    enc.close()


def test_device_resident_input():
    """the pool filled in place (lamehip_batch_pcm_device_ptr + _set_length) and through lamehip_batch_set_pcm_device,
    from a torch tensor; every row holds 0x7fff beyond its stream's length, which must never be read.  In a process of
    its own (tests/resample_device_child.py), where torch takes the device before the library does -- the order every
    torch program has; for both tap counts (31; 32 at a whole-number ratio) and for mono, whose second plane is never
    read."""
    child = os.path.join(helpers.ROOT, "tests", "resample_device_child.py")
    r = subprocess.run([sys.executable, child, "2", "4", "9"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("device-resident input ok") == 3, r.stdout[-3000:]


def test_pipelined_rounds_on_one_batch():
    """pinned mirror + mark + upload + asynchronous encode + fetch, two rounds on the same batch: the second with other
    samples and other lengths (some shorter, one stream left alone), so a stale plan or stale floats would show"""
    case = 2
    rate_in, kw, out, rate_out = CASES[case]
    pcms1, _, packed1, _ = case_data(case)
    order = [3, 0, 5, 2, 1, 6, 7, 4]            # round 2: the lengths change places ...
    pcms2 = [helpers.synth_stream(7900 + s, pcms1[k].shape[1], rate_in, 1.0 / 7) if pcms1[k].shape[1] else pcms1[k]
             for s, k in enumerate(order)]
    keep = 6                                    # ... except for one stream, which is not declared again
    pcms2[keep] = pcms1[keep]
    enc = open_product(rate_in, kw, out, require_device=True)
    off = lamehip.Batch(enc, len(pcms2), max(x.shape[1] for x in pcms1))
    fill(off, pcms2)
    off.encode()
    packed2 = [off.pack(s) for s in range(len(pcms2))]
    off.close()
    assert packed2[keep] == packed1[keep]
    b = device_batch(enc, pcms1)
    for rnd, (pcms, packed) in enumerate(((pcms1, packed1), (pcms2, packed2))):
        h = b.pcm_host()
        for s, x in enumerate(pcms):
            if rnd == 1 and s == keep:
                continue
            h[s, :, :x.shape[1]] = x
            h[s, :, x.shape[1]:] = 0x7fff
            b.set_length(s, x.shape[1])
            b.mark_pcm(s)
        b.upload()
        b.encode(sync=False)
        b.fetch()
        for s, want in enumerate(packed):
            assert bytes(b.bytes_view(s)) == want, (rnd, s)
            assert b.pack(s) == want, (rnd, s)
    b.close()
    enc.close()


def test_ragged_batch_shares_the_trunk():
    """70 short streams of spread lengths (two of them equal) at 48 -> 44.1 kHz: several workgroups per stream, one
    trunk for all; every stream's floats, a sample of the bytes"""
    rate_in, kw, out, rate_out = CASES[2]
    rng = np.random.default_rng(70)
    lens = [int(v) for v in rng.integers(0, int(rate_in * 0.3), 70)]
    lens[41] = lens[17]
    lens[5] = int(rate_in * 0.3)
    pcms = [(rng.standard_normal((2, n)) * 7000).clip(-32768, 32767).astype(np.int16) for n in lens]
    enc = open_product(rate_in, kw, out, require_device=True)
    cfg = enc.config()
    off = lamehip.Batch(enc, len(pcms), max(lens))
    fill(off, pcms)
    off.encode()
    b = device_batch(enc, pcms)
    fill(b, pcms)
    b.encode()
    lib = rsup.library()
    for s, x in enumerate(pcms):
        want = rsup.host_convert(lib, rate_in, rate_out, cfg.channels, cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r, x)[0]
        assert rsup.same_floats(b.converted(s), want), "stream %d" % s
        assert b.frames(s) == off.frames(s)
    for s in (0, 5, 17, 41, 42, 69):
        assert b.pack(s) == off.pack(s), s
        assert b.get_bytes(s) == off.pack(s), s
    off.close()
    b.close()
    enc.close()


def test_window_mode_after_device_conversion(monkeypatch):
    """LAMEHIP_MID_WINDOW=3: the launch behind the conversion runs in windows of frames, same bytes"""
    case = 1
    rate_in, kw, out, rate_out = CASES[case]
    pcms, floats, packed, frames = case_data(case)
    enc = open_product(rate_in, kw, out, require_device=True)
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "3")
    b = device_batch(enc, pcms)
    fill(b, pcms)
    b.encode()
    assert b.windows() > 1
    check_bytes(b, packed)
    b.close()
    enc.close()


def test_refusals():
    lib = lamehip.load_library()
    lib.lamehip_batch_set_device_resampling.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    x = helpers.synth_stream(7990, 3000, 48000)
    # a batch that does not convert
    plain = lamehip.Encoder(44100, 128)
    b = lamehip.Batch(plain, 1, 3000)
    assert lib.lamehip_batch_set_device_resampling(b.b, 1) == -1
    assert b"does not convert" in lib.lamehip_last_error()
    b.close()
    plain.close()
    rate_in, kw, out, rate_out = CASES[2]
    enc = open_product(rate_in, kw, out, require_device=True)
    # after PCM was handed over
    b = lamehip.Batch(enc, 1, 3000)
    b.set_pcm(0, x[0], x[1])
    assert lib.lamehip_batch_set_device_resampling(b.b, 1) == -1
    assert b"before any PCM" in lib.lamehip_last_error()
    # incremental use of a converting batch, switch off ...
    assert lib.lamehip_batch_append(b.b, 0, x[0].ctypes.data, x[1].ctypes.data, 1000) == -1
    b.close()
    # ... and on; a length that does not fit the pool
    b = lamehip.Batch(enc, 1, 3000)
    b.set_device_resampling()
    assert lib.lamehip_batch_append(b.b, 0, x[0].ctypes.data, x[1].ctypes.data, 1000) == -1
    assert lib.lamehip_batch_set_length(b.b, 0, 3000 + 100000) == -1
    assert b"exceeds the pool" in lib.lamehip_last_error()
    assert lib.lamehip_batch_set_pcm(b.b, 0, x[0].ctypes.data, x[1].ctypes.data, 3000) == 0
    assert lib.lamehip_batch_set_device_resampling(b.b, 0) == -1       # PCM is in: the converter's place is settled
    b.encode()
    assert len(b.pack(0)) > 0
    b.close()
    enc.close()
