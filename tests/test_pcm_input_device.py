"""Typed input of a batch on the device (lamehip_batch_set_sample_type, csrc/lh_ingest.hip): int32 and float32 streams give
the bytes of the reference entry point their type is named after -- lame_encode_buffer_int / _float / _ieee_float /
_interleaved* --, through both packers, from host arrays, the pinned mirror and torch tensors on the same GPU, with and
without rate conversion on the device; the floats the kernels read are the host evaluation's bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import lamehip
import pcm_input_support as psup
from lamehip import PCM_DTYPES, PCM_F32, PCM_F32_UNIT, PCM_S16, PCM_S32

pytestmark = pytest.mark.gpu

# (id, sample type, input rate, encoder settings, interleaved, LAMEHIP_MID_WINDOW)
CASES = [
    ("f32unit-cbr128-js", PCM_F32_UNIT, 44100, dict(brate=128, mode=1), False, None),
    ("f32-vbr3", PCM_F32, 44100, dict(vbr_q=3), False, None),
    ("s32-cbr128", PCM_S32, 44100, dict(brate=128), False, None),
    ("s32-mono96", PCM_S32, 44100, dict(brate=96, channels=1), False, None),
    ("f32unit-vbr2-downmix", PCM_F32_UNIT, 44100, dict(vbr_q=2, mode=3), False, None),
    ("f32unit-scales", PCM_F32_UNIT, 44100, dict(brate=128, scale_left=0.7, scale_right=1.3), False, None),
    ("s16-interleaved", PCM_S16, 44100, dict(brate=128), True, None),
    ("f32unit-interleaved", PCM_F32_UNIT, 44100, dict(brate=128), True, None),
    ("f32unit-22k-mpeg2", PCM_F32_UNIT, 22050, dict(brate=64), False, None),
    ("f32-window3", PCM_F32, 44100, dict(brate=128), False, 3),
]
IDS = [c[0] for c in CASES]
# typed input in front of the device rate converter: (id, sample type, input rate, settings, output rate)
RATE_CASES = [("f32unit-48k-44k", PCM_F32_UNIT, 48000, dict(brate=128), 44100), ("s32-22k-44k", PCM_S32, 22050, dict(brate=128), 44100)]


def case_lengths(sr):
    return [int(0.5 * sr) + 13, 5000, 1, 0, 1151, 1152, 1153, 3]


def open_product(sr, kw, out=0):
    enc = lamehip.Encoder.__new__(lamehip.Encoder)
    lib = enc.lib = lamehip.load_library()
    enc.h = C.c_void_p(lib.lame_init())
    enc.channels = kw.get("channels", 2)
    lib.lame_set_in_samplerate(enc.h, sr)
    lib.lame_set_num_channels(enc.h, enc.channels)
    lib.lame_set_bWriteVbrTag(enc.h, 0)
    if out:
        lib.lame_set_out_samplerate(enc.h, out)
    if "brate" in kw:
        lib.lame_set_brate(enc.h, kw["brate"])
    if "vbr_q" in kw:
        lib.lame_set_VBR(enc.h, 4)
        lib.lame_set_VBR_q(enc.h, kw["vbr_q"])
    if "mode" in kw:
        lib.lame_set_mode(enc.h, kw["mode"])
    for name in ("scale_left", "scale_right"):
        if name in kw:
            fn = getattr(lib, "lame_set_" + name)
            fn.argtypes = [C.c_void_p, C.c_float]
            fn(enc.h, kw[name])
    enc.rc = lib.lame_init_params(enc.h)
    assert enc.rc == 0, lamehip.last_error()
    return enc


def open_reference(ref, sr, kw, out=0):
    lib = ref.lib
    lib.refh_option.argtypes = [C.c_char_p, C.c_float]
    lib.refh_option(None, 0)
    if out:
        lib.refh_option(b"out_samplerate", float(out))
    for name in ("scale_left", "scale_right"):
        if name in kw:
            lib.refh_option(name.encode(), kw[name])
    lib.refh_set_channels(kw.get("channels", 2))
    try:
        if "vbr_q" in kw:
            h = lib.refh_open_vbr(sr, kw["vbr_q"], kw.get("mode", -1), -1, out, 0)
        else:
            h = lib.refh_open(sr, kw["brate"], kw.get("mode", -1), -1)
    finally:
        lib.refh_option(None, 0)
        lib.refh_set_channels(2)
    assert h, "reference refused the settings"
    return C.c_void_p(h)


def stream_bytes(stype, interleaved, sr, kw, x, chunk, out=0):
    """what the entry point the sample type is named after makes of stream x fed `chunk' samples per call, then the flush:
    the compiled reference's where it was built (oracle/_ref), else this library's own handle call"""
    kind = psup.REF_KIND[(stype, interleaved)]
    n = x.shape[1]
    buf = C.create_string_buffer(4 * chunk + 16000)
    if helpers.have_reference():
        ref = helpers.Reference()
        h = open_reference(ref, sr, kw, out)

        def call(a, b, m):
            return ref.lib.refh_encode_typed(h, kind, a, b, m, buf, len(buf))

        def flush():
            k = ref.lib.refh_flush(h, buf, len(buf))
            ref.lib.refh_close(h)
            return k
    else:
        enc = open_product(sr, kw, out)
        fn = getattr(enc.lib, psup.HANDLE_CALL[kind])
        fn.restype = C.c_int

        def call(a, b, m):
            return fn(enc.h, a, m, buf, len(buf)) if interleaved else fn(enc.h, a, b, m, buf, len(buf))

        def flush():
            k = enc.lib.lame_encode_flush(enc.h, buf, len(buf))
            enc.close()
            return k
    got = b""
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        if interleaved:
            inter = np.ascontiguousarray(x[:, i:i + m].T)
            k = call(C.c_void_p(inter.ctypes.data), None, m)
        else:
            l, r = np.ascontiguousarray(x[0, i:i + m]), np.ascontiguousarray(x[1, i:i + m])
            k = call(C.c_void_p(l.ctypes.data), C.c_void_p(r.ctypes.data), m)
        assert k >= 0
        got += buf.raw[:k]
    k = flush()
    assert k >= 0
    return got + buf.raw[:k]


@functools.lru_cache(maxsize=None)
def case_data(case):
    """per entry of CASES, computed once: the streams and the bytes expected of each (fed in chunks of 1000)"""
    _, stype, sr, kw, interleaved, _ = CASES[case]
    xs = [psup.typed_signal(stype, 8100 + 10 * case + s, n, sr) for s, n in enumerate(case_lengths(sr))]
    return xs, [stream_bytes(stype, interleaved, sr, kw, x, 1000) for x in xs]


def typed_batch(enc, stype, nstreams, cap, dev_rs=False):
    b = lamehip.Batch(enc, nstreams, cap)
    b.set_device_packing()
    if dev_rs:
        b.set_device_resampling()
    if stype != PCM_S16:
        b.set_sample_type(stype)
    return b


def feed(b, xs, interleaved, mono):
    for s, x in enumerate(xs):
        if interleaved:
            b.set_input(s, interleaved=np.ascontiguousarray(x.T))
        elif mono:
            b.set_input(s, x[0])
        else:
            b.set_input(s, x[0], x[1])


def check_bytes(b, want, what=""):
    for s, w in enumerate(want):
        assert b.pack(s) == w, "%s stream %d (host packer)" % (what, s)
        assert b.get_bytes(s) == w, "%s stream %d (device packer)" % (what, s)


def check_floats(b, enc, stype, xs, interleaved=False):
    """converted(): the float planes the kernels read, against the host evaluation"""
    lib = psup.library()
    cfg = enc.config()
    m = psup.matrix(lib, stype, cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r)
    one_plane = cfg.channels == 1 and cfg.pcm_mix == 0.0
    for s, x in enumerate(xs):
        want = psup.host_ingest(lib, stype, m, x[0], None if one_plane else x[1])
        if cfg.channels == 1:
            want[1] = 0.0
        assert psup.same_floats(b.converted(s), want), "stream %d" % s


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_typed_batch_gives_the_entry_points_bytes(case, monkeypatch):
    _, stype, sr, kw, interleaved, window = CASES[case]
    xs, want = case_data(case)
    assert len(want[0]) > 1000
    if window:
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", str(window))
    enc = open_product(sr, kw)
    b = typed_batch(enc, stype, len(xs), max(x.shape[1] for x in xs) + case % 4)
    feed(b, xs, interleaved, enc.channels == 1)
    b.encode()
    assert b.windows() > 1 if window else b.windows() == 1
    check_bytes(b, want)
    if stype != PCM_S16:
        assert b.ingest_ms() > 0.0 and b.resample_ms() == 0.0
        check_floats(b, enc, stype, xs)
    b.close()
    enc.close()


def test_rounding_to_s16_first_is_another_signal():
    """the same float streams rounded to int16 and fed to an s16 batch: other bytes -- the typed path cannot pass through
    an accidental s16 round trip"""
    differ = 0
    for case in (0, 1):
        _, stype, sr, kw, _, _ = CASES[case]
        xs, want = case_data(case)
        enc = open_product(sr, kw)
        b = lamehip.Batch(enc, len(xs), max(x.shape[1] for x in xs))
        for s, x in enumerate(xs):
            r = np.rint(x.astype(np.float64) * (32767.0 if stype == PCM_F32_UNIT else 1.0)).clip(-32768, 32767).astype(np.int16)
            b.set_pcm(s, r[0], r[1])
        b.encode()
        differ += sum(b.pack(s) != want[s] for s in range(len(xs)))
        b.close()
        enc.close()
    assert differ > 0


def test_device_resident_input_from_torch():
    """float32 [B, 2, cap] on the GPU with NaN beyond each length, in a process of its own where torch takes the device
    first (tests/pcm_input_child.py): in place through pcm_device_ptr + set_length, through set_input on tensor slices, and
    from interleaved [n, 2] tensors -- the bytes of the host-fed batch"""
    child = os.path.join(helpers.ROOT, "tests", "pcm_input_child.py")
    r = subprocess.run([sys.executable, child, "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("device-resident typed input ok") == 3, r.stdout[-3000:]


@pytest.mark.parametrize("case", range(len(RATE_CASES)), ids=[c[0] for c in RATE_CASES])
def test_typed_input_with_device_rate_conversion(case):
    """the converter reads the typed pool itself: the bytes of the typed entry point fed 1152 input samples per call, then the
    flush; no ingest pass"""
    _, stype, sr, kw, out = RATE_CASES[case]
    xs = [psup.typed_signal(stype, 8400 + 10 * case + s, n, sr) for s, n in enumerate(case_lengths(sr))]
    want = [stream_bytes(stype, False, sr, kw, x, 1152, out) for x in xs]
    enc = open_product(sr, kw, out)
    b = typed_batch(enc, stype, len(xs), max(x.shape[1] for x in xs) + 1 + case, dev_rs=True)
    feed(b, xs, False, False)
    b.encode()
    assert b.resample_ms() > 0.0 and b.ingest_ms() == 0.0
    check_bytes(b, want)
    b.close()
    enc.close()


def test_pipelined_rounds_on_a_typed_batch():
    """pinned typed mirror + mark + upload + asynchronous encode + fetch, two rounds on one batch: the second with other
    samples and other lengths, one stream not declared again; then reset + encode without declaring anything"""
    case = 0
    _, stype, sr, kw, _, _ = CASES[case]
    xs1, want1 = case_data(case)
    order = [3, 0, 5, 2, 1, 6, 7, 4]
    keep = 6
    xs2 = [psup.typed_signal(stype, 8700 + s, xs1[k].shape[1], sr) for s, k in enumerate(order)]
    xs2[keep] = xs1[keep]
    want2 = [want1[s] if s == keep else stream_bytes(stype, False, sr, kw, x, 1000) for s, x in enumerate(xs2)]
    enc = open_product(sr, kw)
    cap = max(x.shape[1] for x in xs1) + 3
    b = typed_batch(enc, stype, len(xs1), cap)
    for rnd, (xs, want) in enumerate(((xs1, want1), (xs2, want2))):
        h = b.input_host()
        assert h.dtype == PCM_DTYPES[stype] and h.shape == (len(xs1), 2, cap)
        for s, x in enumerate(xs):
            if rnd == 1 and s == keep:
                continue
            h[s, :, :x.shape[1]] = x
            h[s, :, x.shape[1]:] = np.nan
            b.set_length(s, x.shape[1])
            b.mark_pcm(s)
        b.upload()
        b.encode(sync=False)
        b.fetch()
        for s, w in enumerate(want):
            assert bytes(b.bytes_view(s)) == w, (rnd, s)
            assert b.pack(s) == w, (rnd, s)
        b.sync()
        assert b.ingest_ms() > 0.0
    b.reset()
    b.encode()
    assert b.ingest_ms() == 0.0
    check_bytes(b, want2, "after reset")
    b.close()
    enc.close()


def test_refusals():
    lib = lamehip.load_library()
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.lamehip_batch_pcm_host_ptr.restype = C.c_void_p
    lib.lamehip_batch_pcm_host_ptr.argtypes = [C.c_void_p]
    x = helpers.synth_stream(8990, 3000)
    enc = lamehip.Encoder(44100, 128)
    # after PCM was given
    b = lamehip.Batch(enc, 1, 3000)
    b.set_pcm(0, x[0], x[1])
    assert lib.lamehip_batch_set_sample_type(b.b, PCM_F32) == -1
    assert b"before any PCM" in lib.lamehip_last_error()
    b.close()
    # the calls that take shorts, and a length beyond the capacity, on a typed batch
    b = lamehip.Batch(enc, 1, 3000)
    b.set_sample_type(PCM_F32_UNIT)
    assert lib.lamehip_batch_append(b.b, 0, x[0].ctypes.data, x[1].ctypes.data, 1000) == -1
    assert b"lamehip_batch_append" in lib.lamehip_last_error() and b"s16" in lib.lamehip_last_error()
    assert lib.lamehip_batch_set_pcm(b.b, 0, x[0].ctypes.data, x[1].ctypes.data, 3000) == -1
    assert b"lamehip_batch_set_pcm" in lib.lamehip_last_error() and b"not s16" in lib.lamehip_last_error()
    assert lib.lamehip_batch_pcm_host_ptr(b.b) is None
    assert lib.lamehip_batch_set_length(b.b, 0, 3001) == -1
    assert b"exceeds the pool" in lib.lamehip_last_error()
    f = np.zeros(3001, np.float32)
    with pytest.raises(RuntimeError, match="exceeds the pool"):
        b.set_input(0, f, f)
    b.set_input(0, f[:3000], f[:3000])
    b.encode()
    assert len(b.pack(0)) > 0
    b.close()
    enc.close()
    # a type other than s16 on a batch that converts the rate on the host
    enc = open_product(48000, dict(brate=128), 44100)
    b = lamehip.Batch(enc, 1, 3000)
    assert lib.lamehip_batch_set_sample_type(b.b, PCM_S32) == -1
    assert b"lamehip_batch_set_device_resampling first" in lib.lamehip_last_error()
    b.set_device_resampling()
    b.set_sample_type(PCM_S32)
    lib.lamehip_batch_set_device_resampling.argtypes = [C.c_void_p, C.c_int]
    assert lib.lamehip_batch_set_device_resampling(b.b, 0) == -1
    assert b"s16 only" in lib.lamehip_last_error()
    b.close()
    enc.close()
