"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through the
C ABI of liblamehip.so; the checkers are the committed golden vectors, the CPU
oracle and -- when it travelled with the tree -- the compiled reference."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest

import helpers
import lamehip
from lamehip.types import struct_diff


def _poison_tool():
    """tests/gpu_tools/liblamehip_testtools.so (built by __graft_entry__.build()): garbage in every VGPR,
    in LDS and in scratch memory of the device."""
    return C.CDLL(os.path.join(helpers.ROOT, "tests", "gpu_tools", "liblamehip_testtools.so"))

pytestmark = pytest.mark.gpu


def test_wave_primitives_selftest():
    """DPP reductions / ballot / readlane of csrc/lh_wave.h against a serial LDS evaluation."""
    assert lamehip.load_library().lamehip_selftest() == 0


def _encoder(g, **kw):
    return lamehip.Encoder(**helpers.golden_encoder_kwargs(g), **kw)


VBR_GOLDEN = helpers.golden_names(vbr=True)


@pytest.mark.parametrize("name", helpers.golden_names() + VBR_GOLDEN + helpers.golden_names(kind="abr")
                         + helpers.golden_names(kind="mono"))
def test_batch_payload_and_bytes_match_golden(name):
    g, pcm = helpers.load_golden(name)
    enc = _encoder(g)
    b = lamehip.Batch(enc, 2, pcm.shape[1] + 16)
    b.set_pcm(0, pcm[0], pcm[1])
    b.set_pcm(1, pcm[0], pcm[1])            # same stream twice: both slots must agree
    b.encode()
    frames = b.get_frames(0)
    assert len(frames) == int(g["nframes"])
    mp3 = b.pack(0)
    assert mp3 == b.pack(1)
    helpers.normalize_tables(frames)
    want = [str(x) for x in g["frame_sha256"]]
    bad = [i for i, fr in enumerate(frames) if helpers.frame_sha(fr) != want[i]]
    assert not bad, "frames %s differ from the reference" % bad[:8]
    assert mp3 == g["mp3"].tobytes()
    b.close()
    enc.close()


@pytest.mark.parametrize("name,chunk", [("testcase_wav_cbr128", 1152), ("cbr128_js_44k", 777),
                                        ("cbr320_js_48k_bursts", 4000), ("cbr128_js_44k_silence", 1),
                                        ("testcase_wav_vbr2", 1152), ("vbr4_js_44k_white", 2500),
                                        ("vbr0_js_48k_bursts", 600), ("abr128_js_44k", 1152),
                                        ("abr200_st_48k_bursts", 3000), ("mono_cbr96_44k", 1152),
                                        ("mono_vbr2_44k", 2000),
                                        ("cbr64_js_22k_lsf", 576), ("cbr32_js_16k_bursts_lsf", 1152), ("cbr16_js_8k_lsf", 333),
                                        ("vbr4_js_22k_lsf", 1000), ("abr56_js_22k_lsf", 4000), ("mono_cbr48_22k_lsf", 576),
                                        ("vbrold2_js_24k_lsf", 700)])
def test_lame_encode_buffer_call_sequence(name, chunk):
    """lame_init -> set -> init_params -> N x lame_encode_buffer -> flush, as the
    reference frontend drives it (frontend/lame_main.c:381-470)."""
    g, pcm = helpers.load_golden(name)
    enc = _encoder(g)
    n = pcm.shape[1]
    if chunk == 1:
        n = min(n, 3000)                    # one-sample calls: keep it short
    out = b""
    first = enc.encode(pcm[0][:min(chunk, n)], pcm[1][:min(chunk, n)])
    if chunk <= 576:
        assert first == b""                 # priming: the first call returns 0 bytes
    out += first
    for i in range(chunk, n, chunk):
        out += enc.encode(pcm[0][i:min(n, i + chunk)], pcm[1][i:min(n, i + chunk)])
    out += enc.flush()
    assert enc.flush() == b""               # second flush is a no-op (reference lame.c:2076)
    if n == pcm.shape[1]:
        assert out == g["mp3"].tobytes()
    else:
        ref_like = _encoder(g)
        b = lamehip.Batch(ref_like, 1, n)
        b.set_pcm(0, pcm[0][:n], pcm[1][:n])
        b.encode()
        assert out == b.pack(0)
        b.close()
        ref_like.close()
    enc.close()


def test_ragged_batch_matches_oracle(oracle):
    """Streams of different lengths (incl. empty-ish and non-multiples of 1152) in one launch."""
    enc = lamehip.Encoder(44100, 128)
    cfg, tab = enc.config(), enc.tables()
    lengths = [1, 500, 1152, 1153, 4000, 10000, 22050, 3 * 1152 + 17]
    pcms = [helpers.synth_stream(200 + i, n, 44100, 1.0 / 9) for i, n in enumerate(lengths)]
    b = lamehip.Batch(enc, len(pcms), max(lengths))
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode()
    for s, x in enumerate(pcms):
        got = b.get_frames(s)
        want = oracle.encode_frames(cfg, tab, x)
        assert len(got) == len(want)
        for f in range(len(got)):
            d = struct_diff(want[f], got[f])
            assert not d, (s, f, d[:4])
        assert len(b.pack(s)) > 0
    b.close()
    enc.close()


def test_live_reference_when_available(reference):
    for sr, br, mode, seed in ((44100, 128, None, 31), (48000, 320, 1, 32), (44100, 160, None, 33)):
        pcm = helpers.synth_stream(seed, sr * 2, sr, 1.0 / 11)
        mp3, nf, _, _, _ = reference.encode(pcm, sr, br, -1 if mode is None else mode)
        enc = lamehip.Encoder(sr, br, mode)
        b = lamehip.Batch(enc, 1, pcm.shape[1])
        b.set_pcm(0, pcm[0], pcm[1])
        b.encode()
        assert b.frames(0) == nf
        assert b.pack(0) == mp3
        b.close()
        enc.close()


def test_full_batch_size_properties():
    """BASELINE batch size (1024 streams) at reduced length: size-independent properties.
    (a) determinism: two runs give the same payload; (b) independence: a stream
    encoded alone equals its slot in the batch; (c) CBR accounting: every packed
    stream has exactly the CBR frame bytes and passes the packer's reservoir /
    bit-count checks; (d) duplicated inputs give duplicated outputs."""
    enc = lamehip.Encoder(44100, 128)
    B, n = 1024, 44100
    base = [helpers.synth_stream(300 + i, n, 44100, 1.0 / 5) for i in range(8)]
    b = lamehip.Batch(enc, B, n)
    for s in range(B):
        x = base[s % 8]
        b.set_pcm(s, x[0], x[1])
    b.encode()
    packed = {s: b.pack(s) for s in (0, 1, 7, 8, 9, 511, 1016, 1023)}
    for s in (8, 1016):
        assert packed[s] == packed[0]
    assert packed[9] == packed[1] and packed[1023] == packed[7] and packed[511] == packed[7]
    digest1 = hashlib.sha256(b"".join(bytes(b.get_frames(s)) for s in (0, 100, 1023))).hexdigest()
    b.reset()
    b.encode()
    digest2 = hashlib.sha256(b"".join(bytes(b.get_frames(s)) for s in (0, 100, 1023))).hexdigest()
    assert digest1 == digest2
    # CBR accounting: 128 kb/s at 44.1 kHz = 417 or 418 bytes per frame; the flush pads the last one
    nf = b.frames(0)
    assert abs(len(packed[0]) - nf * 128000 / 8 * 1152 / 44100) < 420
    solo = lamehip.Batch(enc, 1, n)
    solo.set_pcm(0, base[1][0], base[1][1])
    solo.encode()
    assert solo.pack(0) == packed[1]
    solo.close()
    b.close()
    enc.close()


def _full_batch_against_oracle(sr, n, burst_interval, seed0, **enc_kw):
    """1024 DIFFERENT signals of the bench's recipe through one launch: every frame of every stream against the oracle
    (payload structs), and the device packer's bytes against the host packer's for every 16th stream."""
    enc = lamehip.Encoder(sr, **enc_kw)
    cfg, tab = enc.config(), enc.tables()
    orc = helpers.Oracle()
    B = 1024
    pcms = [helpers.synth_stream(seed0 + i, n - 7 * (i % 13), sr, burst_interval) for i in range(B)]
    b = lamehip.Batch(enc, B, n)
    b.set_device_packing()
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode()
    split, _ = b.kernel_parts_ms()
    assert split, "the batch did not go through the split pipeline"
    bad = []
    for s, x in enumerate(pcms):
        got = b.get_frames(s)
        want = orc.encode_frames(cfg, tab, x)
        if len(got) != len(want) or any(struct_diff(want[f], got[f]) for f in range(len(want))):
            bad.append(s)
        elif s % 16 == 0 and b.get_bytes(s) != b.pack(s):
            bad.append(-s - 1)
    b.close()
    enc.close()
    assert not bad, bad[:10]


def test_full_batch_every_stream_matches_oracle():
    """BASELINE config[1]'s batch (1024 streams, CBR 128, 44.1 kHz stereo) with 1024 DIFFERENT signals of the bench's recipe,
    1.5 s each.  The launch is the headline's -- 1024 workgroups, two waves per SIMD, every SIMD shared by two streams -- only
    shorter; `bench.py --full` checks 64 streams of the 60 s launch the same way."""
    _full_batch_against_oracle(44100, 44100 * 3 // 2, 1.0 / 3, 91000, brate=128)


def test_full_batch_every_stream_matches_oracle_vbr2():
    """BASELINE config[2] at full occupancy: 1024 different streams, VBR -V2 (vbr_mtrh), 1.5 s each."""
    _full_batch_against_oracle(44100, 44100 * 3 // 2, 1.0 / 3, 93000, vbr_q=2)


def test_full_batch_every_stream_matches_oracle_cbr320_bursts():
    """BASELINE config[4] at full occupancy: 1024 different streams, 48 kHz joint stereo CBR 320 with 40 bursts a second
    (a transient per granule: the short-block path dominates), 1 s each."""
    _full_batch_against_oracle(48000, 48000, 1.0 / 40, 95000, brate=320, mode=1)


@pytest.mark.parametrize("name", ["testcase_wav_cbr128", "cbr320_js_48k_bursts", "cbr128_js_44k_q0"])
def test_no_dependence_on_uninitialised_device_state(name):
    """Registers, LDS and scratch memory are not cleared between kernels.  Fill all of them
    with garbage (the poison tool of tests/gpu_tools) before every launch: the payload must still be the
    reference's, frame by frame, on the batch path and on the one-launch-per-call path."""
    g, pcm = helpers.load_golden(name)
    enc = _encoder(g)
    lib = enc.lib
    want = [str(x) for x in g["frame_sha256"]]
    for pattern in (0xA5A5A580, 0xFFFFFFFF):
        b = lamehip.Batch(enc, 1, pcm.shape[1] + 16)
        b.set_pcm(0, pcm[0], pcm[1])
        assert _poison_tool().lamehip_test_poison(C.c_uint(pattern)) == 0
        b.encode()
        frames = b.get_frames(0)
        helpers.normalize_tables(frames)
        bad = [i for i, fr in enumerate(frames) if helpers.frame_sha(fr) != want[i]]
        assert not bad, "pattern %#x: frames %s differ from the reference" % (pattern, bad[:8])
        b.close()
    enc.close()
    enc = _encoder(g)
    out = b""
    n = min(pcm.shape[1], 1152 * 40)
    for i in range(0, n, 1152):
        assert _poison_tool().lamehip_test_poison(C.c_uint(0xA5A5A580 + i)) == 0
        out += enc.encode(pcm[0][i:min(n, i + 1152)], pcm[1][i:min(n, i + 1152)])
    ref = g["mp3"].tobytes()
    assert len(out) > 0 and out == ref[:len(out)]
    enc.close()


def _stress_signal(seed, n, sr):
    """Signals picked to reach rarely taken paths: level steps, clipping, DC, silence gaps,
    impulses, one silent channel, anti-phase channels, near-silence."""
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    kind = seed % 8
    x = helpers.synth_stream(500 + seed, n, sr, 1.0 / (3 + seed % 13)).astype(np.float64)
    if kind == 0:
        x *= np.where((np.arange(n) // (sr // 7)) % 2 == 0, 1.0, 0.01)      # level steps
    elif kind == 1:
        x = np.clip(x * 3.0, -32768, 32767)                                 # hard clipping
    elif kind == 2:
        x = x * 0.3 + 9000.0                                                # DC offset
    elif kind == 3:
        x[:, n // 3: n // 3 + sr // 5] = 0                                  # digital silence gap
        x[:, :: sr // 9] = 32767                                            # impulses
    elif kind == 4:
        x[1] = 0                                                            # one silent channel
    elif kind == 5:
        x[1] = -x[0]                                                        # anti-phase (pure side)
    elif kind == 6:
        x = rng.integers(-3, 4, size=(2, n)).astype(np.float64)             # near silence
    else:
        x = rng.standard_normal((2, n)) * (rng.uniform(50, 12000))          # noise at a random level
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("sr,br,mode,q", [(44100, 128, None, None), (44100, 128, None, 0), (48000, 320, 1, None),
                                          (32000, 96, None, None), (44100, 192, 0, None), (44100, 256, None, 2),
                                          (48000, 128, None, 7), (32000, 320, 0, 5), (44100, 112, None, 5), (32000, 128, 0, 9),
                                          (44100, 224, 1, 4)])
def test_stress_signals_match_oracle(oracle, sr, br, mode, q):
    """Bit-exact payload against the oracle over signals that exercise the corners of the
    quantisation loop, for several rates / bit rates / stereo modes / quality levels."""
    enc = lamehip.Encoder(sr, br, mode, q)
    cfg, tab = enc.config(), enc.tables()
    n = int(sr * 1.5)
    pcms = [_stress_signal(s * 8 + k, n - 37 * k, sr) for s in range(2) for k in range(8)]
    b = lamehip.Batch(enc, len(pcms), n)
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode()
    for s, x in enumerate(pcms):
        got = b.get_frames(s)
        want = oracle.encode_frames(cfg, tab, x)
        assert len(got) == len(want)
        for f in range(len(got)):
            d = struct_diff(want[f], got[f])
            assert not d, (s, f, d[:4])
    b.close()
    enc.close()


@pytest.mark.parametrize("sr,vq,mode,q", [(44100, 0, None, None), (48000, 4, 1, None), (32000, 5, None, 5), (44100, 2, 3, 1)])
def test_stress_signals_match_oracle_old_vbr_loop(oracle, sr, vq, mode, q):
    """The same for the old VBR loop (vbr_rh).  Seed 7019 at 44.1 kHz -V0 is a regression case of the randomised hunt
    (tests/fuzz_gpu.py old): a frame whose smoothed perceptual entropy is hugely NEGATIVE, where the reference's exp()
    of the masking adjustment overflows to +inf."""
    enc = lamehip.Encoder(sr, mode=mode, quality=q, vbr_q=vq, vbr_mode=2)
    cfg, tab = enc.config(), enc.tables()
    n = int(sr * 1.5)
    pcms = [_stress_signal(s * 8 + k, n - 37 * k, sr) for s in range(2) for k in range(8)]
    pcms.append(_stress_signal(7019, n - 13 * 19, sr))
    b = lamehip.Batch(enc, len(pcms), n)
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode()
    for s, x in enumerate(pcms):
        got = b.get_frames(s)
        want = oracle.encode_frames(cfg, tab, x)
        assert len(got) == len(want)
        for f in range(len(got)):
            d = struct_diff(want[f], got[f])
            assert not d, (s, f, d[:4])
    b.close()
    enc.close()


def test_pack_all_threads_equals_per_stream_pack():
    """lamehip_batch_pack_all (host threads, one pinned staging buffer each) gives the bytes of
    the per-stream call."""
    enc = lamehip.Encoder(44100, 128)
    lengths = [44100 + 977 * i for i in range(24)] + [1, 1152, 0]
    pcms = [helpers.synth_stream(900 + i, max(n, 1), 44100, 1.0 / 7)[:, :n] for i, n in enumerate(lengths)]
    b = lamehip.Batch(enc, len(pcms), max(lengths))
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode()
    single = [b.pack(s) for s in range(len(pcms))]
    for nt in (1, 5, 64):
        assert b.pack_all(nt) == single
    # a worker's failure reaches the caller: its code and its message (the error text is per thread)
    stride = 512
    buf = np.empty(len(pcms) * stride, dtype=np.uint8)
    sizes = np.zeros(len(pcms), dtype=np.int64)
    rc = b.lib.lamehip_batch_pack_all(b.b, 4, buf.ctypes.data, stride, sizes.ctypes.data)
    assert rc == -1 and (sizes < 0).any()
    assert "out_stride 512 is too small for stream" in lamehip.last_error()
    b.close()
    enc.close()


@pytest.mark.parametrize("pattern", [[50000, 1, 1151, 7, 30000], [0, 3, 0, 20000], [1152] * 3 + [9999]])
def test_odd_call_patterns_match_reference_call_by_call(reference, pattern):
    """Chunk sizes a frontend would not use (one huge call, zero-length calls, single samples),
    then flush twice: every call must return the reference's bytes for the same call."""
    sr, br = 44100, 128
    total = sum(pattern)
    pcm = helpers.synth_stream(4711 + total, max(total, 1), sr, 1.0 / 8)
    lib = reference.lib
    lib.refh_open.restype = C.c_void_p
    h = C.c_void_p(lib.refh_open(sr, br, -1, -1))
    enc = lamehip.Encoder(sr, br)
    buf = C.create_string_buffer(200000)
    pos = 0
    for n in pattern:
        l = np.ascontiguousarray(pcm[0][pos:pos + n])
        r = np.ascontiguousarray(pcm[1][pos:pos + n])
        k = lib.refh_encode(h, l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), n, buf, len(buf))
        assert k >= 0
        want = buf.raw[:k]
        got = enc.encode(l, r) if n > 0 else b""
        assert got == want, ("call with %d samples at %d" % (n, pos))
        pos += n
    k = lib.refh_flush(h, buf, len(buf))
    assert enc.flush() == buf.raw[:k]
    k = lib.refh_flush(h, buf, len(buf))
    assert k == 0 and enc.flush() == b""          # a second flush has nothing left (reference lame.c:2071)
    lib.refh_close(h)
    enc.close()


@pytest.mark.parametrize("sr,vq,mode,seed,white", [(44100, 2, None, 31, False), (44100, 0, 0, 32, False),
                                                   (48000, 5, None, 33, True), (32000, 3, None, 34, False),
                                                   (44100, 9, None, 35, False), (48000, 1, None, 36, True),
                                                   (44100, 6, 0, 37, False)])
@pytest.mark.parametrize("q", [None, 7])
def test_vbr_batch_matches_oracle(sr, vq, mode, seed, white, q, oracle):
    """vbr_mtrh streams of different lengths in one launch against the CPU oracle (every frame's
    payload incl. its bitrate index, and the packed bytes).  -V6 is the one preset whose long and
    short masking adjustments differ (the value the loop leaves for the next frame's psy model)."""
    lens = [int(sr * 1.3), int(sr * 0.4) + 17, 1, int(sr * 0.9)]
    out = sr if vq >= 7 else 0
    enc = lamehip.Encoder(sr, mode=mode, quality=q, vbr_q=vq, out_samplerate=out)   # q 7: guessed scalefactors
    cfg, tab = enc.config(), enc.tables()
    b = lamehip.Batch(enc, len(lens), max(lens))
    pcms = [helpers.synth_stream(seed * 10 + i, n, sr, 1.0 / 9, white and i == 0) for i, n in enumerate(lens)]
    for i, x in enumerate(pcms):
        b.set_pcm(i, x[0], x[1])
    b.encode()
    for i, x in enumerate(pcms):
        want = oracle.encode_frames(cfg, tab, x)
        got = b.get_frames(i)
        assert len(got) == len(want)
        for f in range(len(want)):
            d = struct_diff(want[f], got[f])
            assert not d, (i, f, d[:4])
        assert b.pack(i) == helpers.pack_frames(enc.lib, cfg, tab, want)
    b.close()
    enc.close()


@pytest.mark.parametrize("sr,kb,mode,q,seed,white", [(44100, 128, None, None, 41, False), (48000, 245, 0, None, 42, False),
                                                     (32000, 100, None, 5, 43, True), (44100, 320, None, 0, 44, False),
                                                     (44100, 160, None, 7, 45, False)])
def test_abr_batch_matches_oracle(sr, kb, mode, q, seed, white, oracle):
    """ABR (--abr n) streams of different lengths in one launch against the CPU oracle."""
    lens = [int(sr * 1.1), int(sr * 0.35) + 5, 1, int(sr * 0.8)]
    enc = lamehip.Encoder(sr, mode=mode, quality=q, abr=kb)
    cfg, tab = enc.config(), enc.tables()
    b = lamehip.Batch(enc, len(lens), max(lens))
    pcms = [helpers.synth_stream(seed * 10 + i, n, sr, 1.0 / 9, white and i == 0) for i, n in enumerate(lens)]
    for i, x in enumerate(pcms):
        b.set_pcm(i, x[0], x[1])
    b.encode()
    for i, x in enumerate(pcms):
        want = oracle.encode_frames(cfg, tab, x)
        got = b.get_frames(i)
        assert len(got) == len(want)
        for f in range(len(want)):
            d = struct_diff(want[f], got[f])
            assert not d, (i, f, d[:4])
        assert b.pack(i) == helpers.pack_frames(enc.lib, cfg, tab, want)
    b.close()
    enc.close()


@pytest.mark.parametrize("kw", [dict(brate=128), dict(brate=320, samplerate=48000), dict(vbr_q=2), dict(vbr_q=5, quality=5),
                                dict(abr=160), dict(vbr_q=0, samplerate=48000),
                                dict(brate=64, samplerate=22050), dict(vbr_q=5, samplerate=24000), dict(abr=40, samplerate=16000),
                                dict(brate=32, samplerate=12000), dict(vbr_q=4, samplerate=22050, vbr_mode=2)])
def test_long_streams_match_oracle(kw, oracle):
    """20 s per stream (765+ frames): reservoir, bitrate switching and the psy history over a length
    that the short fixtures do not reach; bytes and every frame's payload against the CPU oracle."""
    sr = kw.get("samplerate", 44100)
    enc = lamehip.Encoder(**kw)
    cfg, tab = enc.config(), enc.tables()
    n = sr * 20
    pcms = [helpers.synth_stream(900 + i, n - 1000 * i, sr, 1.0 / (3 + 4 * i), white=(i == 2)) for i in range(3)]
    b = lamehip.Batch(enc, len(pcms), n)
    for i, x in enumerate(pcms):
        b.set_pcm(i, x[0], x[1])
    b.encode()
    for i, x in enumerate(pcms):
        want = oracle.encode_frames(cfg, tab, x)
        got = b.get_frames(i)
        assert len(got) == len(want)
        bad = [f for f in range(len(want)) if struct_diff(want[f], got[f])]
        assert not bad, (i, bad[:5])
        assert b.pack(i) == helpers.pack_frames(enc.lib, cfg, tab, want)
    b.close()
    enc.close()


@pytest.mark.parametrize("kw", [dict(brate=128), dict(brate=64, samplerate=32000), dict(brate=320, samplerate=48000, quality=0),
                                dict(vbr_q=0, samplerate=48000), dict(vbr_q=4), dict(vbr_q=7, quality=7), dict(abr=90),
                                dict(abr=256, quality=5), dict(brate=32, samplerate=22050), dict(vbr_q=6, samplerate=16000),
                                dict(brate=16, samplerate=8000)])
def test_mono_batch_matches_oracle(kw, oracle):
    """One input channel (MPEG mode mono): ragged batch against the CPU oracle, every frame and the bytes."""
    sr = kw.get("samplerate", 44100)
    if kw.get("vbr_q", 0) >= 7:
        kw = dict(kw, out_samplerate=sr)
    enc = lamehip.Encoder(channels=1, **kw)
    cfg, tab = enc.config(), enc.tables()
    lens = [int(sr * 1.2), int(sr * 0.3) + 11, 1, int(sr * 0.7)]
    b = lamehip.Batch(enc, len(lens), max(lens))
    pcms = [helpers.synth_stream(1200 + i, n, sr, 1.0 / 8, white=(i == 3)) for i, n in enumerate(lens)]
    for i, x in enumerate(pcms):
        b.set_pcm(i, x[0])
    b.encode()
    for i, x in enumerate(pcms):
        want = oracle.encode_frames(cfg, tab, np.stack([x[0], x[0]]))
        got = b.get_frames(i)
        assert len(got) == len(want)
        bad = [f for f in range(len(want)) if struct_diff(want[f], got[f])]
        assert not bad, (i, bad[:5])
        assert b.pack(i) == helpers.pack_frames(enc.lib, cfg, tab, want)
    b.close()
    enc.close()


@pytest.mark.parametrize("kw", [dict(brate=128), dict(vbr_q=2), dict(abr=120, samplerate=48000)])
def test_downmix_to_mono_matches_oracle(kw, oracle):
    """Two input channels, MPEG mode MONO: the window is l * m00 + r * m01 (reference lame.c:1224-1229)."""
    sr = kw.get("samplerate", 44100)
    enc = lamehip.Encoder(mode=3, **kw)
    cfg, tab = enc.config(), enc.tables()
    assert cfg.channels == 1 and cfg.pcm_mix != 0
    n = int(sr * 0.9)
    x = helpers.synth_stream(1300, n, sr, 1.0 / 6)
    b = lamehip.Batch(enc, 1, n)
    b.set_pcm(0, x[0], x[1])
    b.encode()
    want = oracle.encode_frames(cfg, tab, x)
    got = b.get_frames(0)
    assert len(got) == len(want)
    bad = [f for f in range(len(want)) if struct_diff(want[f], got[f])]
    assert not bad, bad[:5]
    out = b"".join(enc.encode(x[0][i:i + 1152], x[1][i:i + 1152]) for i in range(0, n, 1152)) + enc.flush()
    assert out == b.pack(0) == helpers.pack_frames(enc.lib, cfg, tab, want)
    b.close()
    enc.close()


@pytest.mark.parametrize("kw", [dict(brate=160), dict(vbr_q=3, samplerate=48000), dict(abr=128)])
def test_dual_channel_uncoupled_blocks_match_oracle(kw, oracle):
    """MPEG mode 2: two independent channels, attacks in the left one only, so that the channels of a
    granule take different block types (never the case in the stereo modes, which couple them)."""
    sr = kw.get("samplerate", 44100)
    enc = lamehip.Encoder(mode=2, **kw)
    cfg, tab = enc.config(), enc.tables()
    n = int(sr * 1.0)
    x = helpers.synth_stream(99, n, sr, 1.0 / 11)
    pcm = np.stack([x[0], (8000 * np.sin(2 * np.pi * 440 * np.arange(n) / sr)).astype(np.int16)])
    b = lamehip.Batch(enc, 1, n)
    b.set_pcm(0, pcm[0], pcm[1])
    b.encode()
    want = oracle.encode_frames(cfg, tab, pcm)
    got = b.get_frames(0)
    assert sum(fr.gr[g][0].block_type != fr.gr[g][1].block_type for fr in want for g in range(2)) > 5
    bad = [f for f in range(len(want)) if struct_diff(want[f], got[f])]
    assert len(got) == len(want) and not bad, bad[:5]
    assert b.pack(0) == helpers.pack_frames(enc.lib, cfg, tab, want)
    b.close()
    enc.close()


@pytest.mark.skipif(not helpers.have_reference(), reason="needs oracle/_ref (reference sources)")
@pytest.mark.parametrize("kind,kw", [(1, dict(brate=128)), (2, dict(vbr_q=3)), (3, dict(brate=160)), (4, dict(abr=140)),
                                     (5, dict(brate=128)), (6, dict(vbr_q=5)), (7, dict(brate=192)), (8, dict(brate=128)),
                                     (5, dict(brate=96, channels=1)), (2, dict(vbr_q=2, mode=3))])
def test_typed_buffer_entry_points_match_reference(kind, kw):
    """lame_encode_buffer_float / _ieee_float / _interleaved_ieee_float / _ieee_double / _int / _long / _long2 /
    _interleaved, call by call against the compiled reference fed the very same buffers (samples that are
    not whole 16-bit steps included: the window is float from the host on)."""
    import ctypes as C
    sr, n, chunk = 44100, 44100, 1000
    rng = np.random.Generator(np.random.PCG64(kind))
    x = helpers.synth_stream(1500 + kind, n, sr, 1.0 / 7).astype(np.float64) + rng.uniform(-0.4, 0.4, (2, n))
    if kind in (2, 3, 4):
        x = x / 32767.0
    dt = {1: np.float32, 2: np.float32, 3: np.float32, 4: np.float64, 5: np.int32, 6: np.int64, 7: np.int64, 8: np.int16}[kind]
    if kind == 5:
        x = x * 65536.0
    if kind == 7:
        x = x * 2.0 ** 48
    x = np.ascontiguousarray(x.astype(dt))
    name = {1: "lame_encode_buffer_float", 2: "lame_encode_buffer_ieee_float", 3: "lame_encode_buffer_interleaved_ieee_float",
            4: "lame_encode_buffer_ieee_double", 5: "lame_encode_buffer_int", 6: "lame_encode_buffer_long",
            7: "lame_encode_buffer_long2", 8: "lame_encode_buffer_interleaved"}[kind]
    ref = helpers.Reference().lib
    nch = kw.get("channels", 2)
    ref.refh_set_channels(nch)
    mode = kw.get("mode", -1)
    if "vbr_q" in kw:
        rh = ref.refh_open_vbr(sr, kw["vbr_q"], mode, -1, 0, 0)
    elif "abr" in kw:
        rh = ref.refh_open_abr(sr, kw["abr"], mode, -1, 0, 0)
    else:
        rh = ref.refh_open(sr, kw["brate"], mode, -1)
    ref.refh_set_channels(2)
    assert rh
    rh = C.c_void_p(rh)
    enc = lamehip.Encoder(sr, **kw)
    fn = getattr(enc.lib, name)
    fn.restype = C.c_int
    buf = C.create_string_buffer(2 * chunk + 8000)
    rbuf = C.create_string_buffer(2 * chunk + 8000)
    mine = theirs = b""
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        if kind in (3, 8):
            inter = np.ascontiguousarray(x[:, i:i + m].T.reshape(-1))
            a = (C.c_void_p(inter.ctypes.data), None)
        else:
            a = (C.c_void_p(x[0, i:].ctypes.data), C.c_void_p(x[1, i:].ctypes.data))
        if kind in (3, 8):
            k1 = fn(enc.h, a[0], m, buf, len(buf))
        else:
            k1 = fn(enc.h, a[0], a[1], m, buf, len(buf))
        k2 = ref.refh_encode_typed(rh, kind, a[0], a[1], m, rbuf, len(rbuf))
        assert k1 == k2 >= 0, (i, k1, k2, lamehip.last_error())
        mine += buf.raw[:k1]
        theirs += rbuf.raw[:k2]
    k2 = ref.refh_flush(rh, rbuf, len(rbuf))
    theirs += rbuf.raw[:k2]
    mine += enc.flush()
    ref.refh_close(rh)
    assert mine == theirs and len(mine) > 1000
    enc.close()


@pytest.mark.parametrize("name", helpers.golden_names() + helpers.golden_names(vbr=True) + helpers.golden_names(kind="abr")
                         + helpers.golden_names(kind="mono"))
def test_device_bit_packer_matches_golden(name):
    """lamehip_batch_set_device_packing: the kernel assembles the MP3 bytes itself (lh_dev_emit.h); they equal
    the reference's bytes and the host packer's."""
    g, pcm = helpers.load_golden(name)
    enc = _encoder(g)
    b = lamehip.Batch(enc, 3, pcm.shape[1] + 16)
    b.set_device_packing()
    b.set_pcm(0, pcm[0], pcm[1])
    b.set_pcm(1, pcm[0][:pcm.shape[1] // 3], pcm[1][:pcm.shape[1] // 3])
    b.set_pcm(2, pcm[0][:1], pcm[1][:1])
    b.encode()
    assert b.get_bytes(0) == g["mp3"].tobytes() == b.pack(0)
    assert b.get_bytes(1) == b.pack(1)
    assert b.get_bytes(2) == b.pack(2)
    b.reset()                       # a second run over the same batch starts from clean packer state
    b.encode()
    assert b.get_bytes(0) == g["mp3"].tobytes()
    b.close()
    enc.close()


@pytest.mark.parametrize("kw", [dict(brate=128), dict(vbr_q=2), dict(abr=160, channels=1), dict(brate=32, samplerate=32000,
                                                                                             out_samplerate=32000)])
def test_device_bit_packer_long_streams(kw):
    """30 s streams, many frames of reservoir back pointers; 32 kb/s has the smallest frames (a 511-byte
    back pointer then spans several headers)."""
    sr = kw.get("samplerate", 44100)
    enc = lamehip.Encoder(**kw)
    n = sr * 30
    pcms = [helpers.synth_stream(2000 + i, n - 777 * i, sr, 1.0 / (2 + 3 * i), white=(i == 1)) for i in range(3)]
    b = lamehip.Batch(enc, len(pcms), n)
    b.set_device_packing()
    for i, x in enumerate(pcms):
        b.set_pcm(i, x[0], x[1])
    b.encode()
    for i in range(len(pcms)):
        assert b.get_bytes(i) == b.pack(i)
    b.close()
    enc.close()


@pytest.mark.gpu
def test_device_bit_packer_holds_every_pending_header_of_the_smallest_frames():
    """24 kHz, 8 kb/s, stereo, CRC: frames of 24 bytes with 23 of header + side information, one byte of main data each --
    digital silence fills the 255-byte reservoir, so up to 255 frame headers lie inside one stretch of main data.  The
    device packer's queue of pending headers holds 256 like the host packer's and the reference's (MAX_HEADER_BUF); with
    128 the kernel raised status bit 8 and the stream was refused."""
    enc = lamehip.Encoder(24000, 8, error_protection=True)
    n = 24000 * 20
    pcms = [np.zeros((2, n), np.int16), helpers.synth_stream(77, n, 24000, 0.25)]
    pcms[1][:, n // 3:] = 0                             # music, then silence
    b = lamehip.Batch(enc, len(pcms), n)
    b.set_device_packing()
    for i, x in enumerate(pcms):
        b.set_pcm(i, x[0], x[1])
    b.encode()
    for i in range(len(pcms)):
        assert b.get_bytes(i) == b.pack(i)
    b.close()
    enc.close()


@pytest.mark.gpu
def test_bench_spawns_its_own_ranks():
    """python bench.py --gpus 2 without a launcher: two ranks (sharing this box's device when it has
    one), a file barrier, ONE JSON line with the aggregate of both."""
    import json
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "2", "--streams", "16",
                          "--seconds", "2", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900,
                         env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["streams_per_gpu"] == 16
    assert res["checked_against_oracle"]["result"] == "identical"


@pytest.mark.gpu
def test_bench_eight_ranks_shard_a_batch_without_any_collective():
    """BASELINE config[3]'s shape in small: python bench.py --gpus 8 --streams 32 (eight ranks, oversubscribing this
    box's device when it has only one): ONE JSON line, n_gpus 8, the eight ranks' blocks are distinct, contiguous and
    cover streams 0..255 of the global batch, every rank reports its own timing, nothing crosses ranks but timing
    scalars (no collective on the data path), and the rank processes need (next to) no host CPU while their kernels
    run -- eight of them fit the 16-CPU container the pool's boxes give --, and every rank checks streams of its own block
    against the oracle."""
    import json
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "8", "--streams", "32",
                          "--seconds", "2", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500,
                         env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 8 and res["config"]["streams_per_gpu"] == 32 and res["scaling"] == "weak"
    assert res["collectives_on_data_path"] == 0
    ranks = sorted(res["per_rank"], key=lambda r: r["rank"])
    assert [r["rank"] for r in ranks] == list(range(8))
    assert [tuple(r["streams"]) for r in ranks] == [(32 * k, 32 * k + 32) for k in range(8)]
    assert all(r["value"] > 0 and r["kernel_ms_avg"] > 0 for r in ranks)
    # whole-job value = all ranks' audio over the slowest rank's time
    slowest = max(r["s_per_step"] for r in ranks)
    assert res["value"] <= 8 * 32 * 2.0 / slowest * 1.001
    assert res["checked_against_oracle"]["result"] == "identical"
    # every rank compared streams of ITS OWN block with the oracle (on a node with eight devices: each device's output)
    assert all(r["checked"] == "identical" and r["checked_streams"] >= 2 for r in ranks), ranks
    # the host side of a rank during the timed region: it sleeps on a blocking event while its kernels run
    # (lamehip_batch_sync), so eight ranks do not take eight CPUs
    assert all(r["host_cpu_per_wall_s"] <= 0.6 for r in ranks), ranks      # (a rank that spun would show 1.0; a loaded host moves the figure)


@pytest.mark.gpu
def test_bench_under_the_torch_launcher():
    """The command the driver uses for N > 1: python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2
    (one rank per GPU; on a 1-GPU box both ranks share the device).  Rank 0 prints ONE JSON line with the
    aggregate; the ranks only meet in gloo for the barrier and the maximum of the times."""
    import json
    import subprocess
    import sys
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29677", os.path.join(helpers.ROOT, "bench.py"),
           "--gpus", "2", "--streams", "16", "--seconds", "2", "--steps", "1", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--no-extras"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900,
                         env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["streams_per_gpu"] == 16 and res["scaling"] == "weak"
    assert res["checked_against_oracle"]["result"] == "identical"


@pytest.mark.gpu
def test_batch_on_named_device_and_reuse():
    """lamehip_batch_create_on + a batch encoded twice with different PCM equals fresh batches (the
    carried state starts over by itself)."""
    g, pcm = helpers.load_golden("cbr128_js_44k")
    enc = lamehip.Encoder(require_device=True, device=0, **helpers.golden_encoder_kwargs(g))
    n = pcm.shape[1]
    other = helpers.synth_stream(4242, n)
    b = lamehip.Batch(enc, 2, n, device=0)
    fresh = []
    for x in (pcm, other):
        f = lamehip.Batch(enc, 1, n)
        f.set_pcm(0, x[0], x[1])
        f.encode(sync=True)
        fresh.append(f.pack(0))
        f.close()
    b.set_pcm(0, pcm[0], pcm[1])
    b.set_pcm(1, other[0], other[1])
    b.encode(sync=True)
    assert b.pack(0) == fresh[0] and b.pack(1) == fresh[1]
    b.set_pcm(0, other[0], other[1])
    b.set_pcm(1, pcm[0], pcm[1])
    b.encode(sync=True)             # no reset() in between
    assert b.pack(0) == fresh[1] and b.pack(1) == fresh[0]
    assert fresh[0] == g["mp3"].tobytes()
    b.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(brate=128), dict(vbr_q=2)])
def test_incremental_batch_matches_reference_call_by_call(reference, kw):
    """lamehip_batch_append / _encode_available / _drain: eight streams fed in ragged chunks (also
    empty ones), one launch per round; what every stream drains after a round is what the
    reference's lame_encode_buffer returns for that stream's call of the round, and
    lamehip_batch_finish is its lame_encode_flush."""
    sr, B = 44100, 8
    rng = np.random.default_rng(77)
    lens = [int(sr * 0.9) + 37 * s for s in range(B)]
    pcms = [helpers.synth_stream(600 + s, lens[s], sr, 1.0 / 7) for s in range(B)]
    lib = reference.lib
    lib.refh_open.restype = C.c_void_p
    lib.refh_open_vbr.restype = C.c_void_p
    if "vbr_q" in kw:
        hs = [C.c_void_p(lib.refh_open_vbr(sr, kw["vbr_q"], -1, -1, 0, 0)) for _ in range(B)]
    else:
        hs = [C.c_void_p(lib.refh_open(sr, kw["brate"], -1, -1)) for _ in range(B)]
    enc = lamehip.Encoder(sr, **kw)
    b = lamehip.Batch(enc, B, max(lens) + 16)
    buf = C.create_string_buffer(400000)
    pos = [0] * B
    rounds = 0
    while any(pos[s] < lens[s] for s in range(B)):
        want = []
        for s in range(B):
            n = int(rng.choice([0, 1, 575, 1152, 1153, 4000, 9000]))
            n = min(n, lens[s] - pos[s])
            l = np.ascontiguousarray(pcms[s][0][pos[s]:pos[s] + n])
            r = np.ascontiguousarray(pcms[s][1][pos[s]:pos[s] + n])
            k = lib.refh_encode(hs[s], l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), n, buf, len(buf))
            assert k >= 0
            want.append(buf.raw[:k])
            if n:
                b.append(s, l, r)
            pos[s] += n
        b.encode_available()
        for s in range(B):
            assert b.drain(s) == want[s], "round %d stream %d" % (rounds, s)
        rounds += 1
    b.finish()
    for s in range(B):
        k = lib.refh_flush(hs[s], buf, len(buf))
        assert b.drain(s) == buf.raw[:k], "flush of stream %d" % s
        lib.refh_close(hs[s])
    assert rounds > 3
    b.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(brate=128), dict(vbr_q=2), dict(brate=64, samplerate=22050)])
def test_batch_on_the_fused_kernel_matches_oracle(kw, monkeypatch):
    """LAMEHIP_FUSED=1: the batch takes the single fused kernel (the handle API's; also what a launch falls back to when the
    split pipeline's pools cannot be had) -- payload == oracle, frame by frame, and the launch reports no kernel parts."""
    monkeypatch.setenv("LAMEHIP_FUSED", "1")
    kw = dict(kw)
    sr = kw.pop("samplerate", 44100)
    enc = lamehip.Encoder(sr, **kw)
    cfg, tab = enc.config(), enc.tables()
    orc = helpers.Oracle()
    pcms = [helpers.synth_stream(4100 + i, sr + 97 * i, sr, 1.0 / (3 + 5 * i)) for i in range(6)]
    b = lamehip.Batch(enc, len(pcms), max(x.shape[1] for x in pcms))
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode()
    split, _ = b.kernel_parts_ms()
    assert not split
    for s, x in enumerate(pcms):
        got, want = b.get_frames(s), orc.encode_frames(cfg, tab, x)
        assert len(got) == len(want)
        for f in range(len(want)):
            d = struct_diff(want[f], got[f])
            assert not d, (s, f, d[:4])
    b.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw,window", [(dict(brate=128), 7), (dict(brate=128), 16), (dict(vbr_q=2), 5), (dict(vbr_q=4, vbr_mode=2), 9),
                                       (dict(abr=150), 11), (dict(brate=320, samplerate=48000, mode=1), 3),
                                       (dict(brate=64, samplerate=22050), 13), (dict(brate=96, channels=1), 6)])
def test_launch_in_frame_windows_matches_oracle(kw, window, monkeypatch):
    """LAMEHIP_MID_WINDOW=n: the split pipeline works through the launch in windows of n frames per stream (what a launch
    whose analysis records do not fit the device's memory does by itself) -- a ragged batch (one stream shorter than a window,
    one empty beyond its priming, bursts that switch blocks across window edges): payload == oracle frame by frame, the
    device packer's bytes == the host packer's, the kernel parts add up to the launch."""
    kw = dict(kw)
    sr = kw.pop("samplerate", 44100)
    ch = kw.get("channels", 2)
    enc = lamehip.Encoder(sr, **kw)
    cfg, tab = enc.config(), enc.tables()
    orc = helpers.Oracle()
    fs = 1152 if sr >= 32000 else 576
    lens = [fs * 41 + 17, fs * 3, fs * 23 + 500, 1, fs * 64, fs * 30 + 1]
    pcms = [helpers.synth_stream(5100 + i, n, sr, 1.0 / (3 + 4 * i)) for i, n in enumerate(lens)]
    if ch == 1:
        pcms = [np.stack([x[0], x[0]]) for x in pcms]
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", str(window))
    for dev_pack in (False, True):
        b = lamehip.Batch(enc, len(pcms), max(lens) + 16)
        if dev_pack:
            b.set_device_packing(True)
        for s, x in enumerate(pcms):
            if ch == 1:
                b.set_pcm(s, x[0])
            else:
                b.set_pcm(s, x[0], x[1])
        b.encode()
        nf = max(b.frames(s) for s in range(len(pcms)))
        assert b.windows() == (nf + window - 1) // window and b.windows() > 1
        split, parts = b.kernel_parts_ms()
        assert split and all(p > 0 for p in parts) and abs(sum(parts) - b.kernel_ms()) < 0.05 * b.kernel_ms() + 0.2
        for s, x in enumerate(pcms):
            got, want = b.get_frames(s), orc.encode_frames(cfg, tab, x)
            assert len(got) == len(want)
            for f in range(len(want)):
                d = struct_diff(want[f], got[f])
                assert not d, (s, f, d[:4])
            if dev_pack:
                assert b.get_bytes(s) == b.pack(s), s
        # the same batch once more, all at once: the launch goes back to one window and the same payload
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", "0")
        first = [b.pack(s) for s in range(len(pcms))]
        b.encode()
        assert b.windows() == 1
        assert [b.pack(s) for s in range(len(pcms))] == first
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", str(window))
        b.close()
    enc.close()


@pytest.mark.gpu
def test_window_size_follows_the_free_memory(monkeypatch):
    """LAMEHIP_MID_BUDGET_MB stands for a device with little memory left: the launch's analysis records (34 368 B per frame)
    do not fit, so the launch runs in windows of as many frames per stream as do; with room for fewer than 64 frames per
    stream it takes the fused kernel and lamehip_last_error() says why.  The bytes are the same either way."""
    sr, B, secs = 44100, 48, 3.0
    enc = lamehip.Encoder(sr, 128)
    n = int(sr * secs)
    pcms = [helpers.synth_stream(5500 + s, n, sr, 1.0 / 6) for s in range(B)]
    b = lamehip.Batch(enc, B, n + 16)
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    b.encode()
    assert b.windows() == 1 and b.kernel_parts_ms()[0]
    want = [b.pack(s) for s in range(B)]
    nf = b.frames(0)
    rec = 34368
    b.close()
    # room for ~80 frames per stream (0.8 of the budget counts, 64 records are kept spare)
    for budget_frames, kind in ((80, "windows"), (40, "fused")):
        monkeypatch.setenv("LAMEHIP_MID_BUDGET_MB", str(int((budget_frames * B + 64) * rec / 0.8 / 1e6) + 1))
        b = lamehip.Batch(enc, B, n + 16)
        for s, x in enumerate(pcms):
            b.set_pcm(s, x[0], x[1])
        b.encode()
        split, _ = b.kernel_parts_ms()
        if kind == "windows":
            assert split and 1 < b.windows() <= (nf + 63) // 64 and b.windows() >= (nf + budget_frames + 1) // (budget_frames + 2), b.windows()
        else:
            assert not split and b.windows() == 1
            assert "fused kernel" in lamehip.last_error(), lamehip.last_error()
        assert [b.pack(s) for s in range(B)] == want, kind
        b.close()
    enc.close()


@pytest.mark.gpu
def test_incremental_batch_in_frame_windows(monkeypatch):
    """An incremental batch whose launches run in windows (every other one): the bytes are the one-shot batch's."""
    sr, B = 44100, 4
    enc = lamehip.Encoder(sr, 128)
    lens = [sr + 4111 * s for s in range(B)]
    pcms = [helpers.synth_stream(5300 + s, lens[s], sr, 1.0 / 4) for s in range(B)]
    one = lamehip.Batch(enc, B, max(lens) + 16)
    for s, x in enumerate(pcms):
        one.set_pcm(s, x[0], x[1])
    one.encode()
    want = [one.pack(s) for s in range(B)]
    one.close()
    b = lamehip.Batch(enc, B, max(lens) + 16)
    got = [b""] * B
    pos, rnd, wins = 0, 0, []
    while pos < max(lens):
        n = 9000 + 1152 * (rnd % 3)
        for s in range(B):
            a, e = min(pos, lens[s]), min(pos + n, lens[s])
            if e > a:
                b.append(s, np.ascontiguousarray(pcms[s][0][a:e]), np.ascontiguousarray(pcms[s][1][a:e]))
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", "3" if rnd % 2 else "0")
        b.encode_available()
        wins.append(b.windows())
        for s in range(B):
            got[s] += b.drain(s)
        pos += n
        rnd += 1
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "2")
    b.finish()
    for s in range(B):
        got[s] += b.drain(s)
        assert got[s] == want[s], s
    assert max(wins) > 1 and min(wins) == 1, wins
    b.close()
    enc.close()


@pytest.mark.gpu
def test_incremental_batch_changes_kernels_between_launches(monkeypatch):
    """An incremental batch whose launches alternate between the split pipeline and the fused kernel (LAMEHIP_SPLIT_DENY=1
    stands for a pool allocation that failed mid-stream): either kernel leaves the stream state as the other expects it, the
    bytes are the one-shot batch's."""
    sr, B = 44100, 5
    enc = lamehip.Encoder(sr, 128)
    lens = [sr + 311 * s for s in range(B)]
    pcms = [helpers.synth_stream(4300 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    one = lamehip.Batch(enc, B, max(lens) + 16)
    for s, x in enumerate(pcms):
        one.set_pcm(s, x[0], x[1])
    one.encode()
    want = [one.pack(s) for s in range(B)]
    one.close()
    b = lamehip.Batch(enc, B, max(lens) + 16)
    got = [b""] * B
    pos, rnd, kinds = 0, 0, []
    while pos < max(lens):
        n = 7000 + 1152 * (rnd % 3)
        for s in range(B):
            a, e = min(pos, lens[s]), min(pos + n, lens[s])
            if e > a:
                b.append(s, np.ascontiguousarray(pcms[s][0][a:e]), np.ascontiguousarray(pcms[s][1][a:e]))
        monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "1" if rnd % 2 else "0")
        b.encode_available()
        kinds.append(bool(b.kernel_parts_ms()[0]))
        for s in range(B):
            got[s] += b.drain(s)
        pos += n
        rnd += 1
    monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "0")
    b.finish()
    for s in range(B):
        got[s] += b.drain(s)
        assert got[s] == want[s], s
    assert True in kinds and False in kinds, kinds
    b.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(brate=128), dict(vbr_q=2), dict(abr=160, channels=1)])
def test_pipelined_batches_pinned_upload_and_fetch(kw):
    """lamehip_batch_pcm_host_ptr / _mark_pcm / _upload / _fetch / _bytes_ptr: three batch objects in flight, reused
    for a second round with other streams; ragged lengths (one row empty); the device-packed bytes that come back
    through the pinned buffers equal the host packer's, and a batch filled through lamehip_batch_set_pcm (which
    now copies into the same mirror) gives the same bytes."""
    enc = lamehip.Encoder(**kw)
    sr, cap = 44100, 44100 * 2
    lens = [cap, cap - 777, 0, 5000]
    objs = [lamehip.Batch(enc, len(lens), cap) for _ in range(3)]
    for b in objs:
        b.set_device_packing()
    for rnd in range(2):
        pcms = [[helpers.synth_stream(300 + 16 * rnd + 4 * k + i, n, sr) if n else np.zeros((2, 0), np.int16)
                 for i, n in enumerate(lens)] for k in range(3)]
        for k, b in enumerate(objs):
            h = b.pcm_host()
            for s, x in enumerate(pcms[k]):
                h[s, :, :x.shape[1]] = x
                b.set_length(s, x.shape[1])
                b.mark_pcm(s)
            b.upload()
            b.encode(sync=False)
            b.fetch()
        for k, b in enumerate(objs):
            for s in range(len(lens)):
                assert bytes(b.bytes_view(s)) == b.pack(s), (rnd, k, s)
    ref = lamehip.Batch(enc, len(lens), cap)
    for s, x in enumerate(pcms[2]):
        ref.set_pcm(s, x[0], x[1] if enc.channels == 2 else None)
    ref.encode()
    for s in range(len(lens)):
        assert ref.pack(s) == bytes(objs[2].bytes_view(s)), s
    ref.close()
    for b in objs:
        b.close()
    enc.close()


@pytest.mark.gpu
def test_incremental_batch_lifecycle_and_large_chunks():
    """lamehip_batch_append with nothing (first call), with one chunk larger than the staging arena allows in one
    piece (60 s: split and flushed on the way), interleaved small chunks; the bytes equal the one-shot batch's.
    After lamehip_batch_finish the batch refuses append / encode_available / finish / encode until
    lamehip_batch_reset, after which the same input gives the same bytes again."""
    enc = lamehip.Encoder(44100, brate=128)
    n_long, n_short = 44100 * 60, 44100 * 2 + 123
    x0 = helpers.synth_stream(501, 44100 * 5)
    x0 = np.tile(x0, (1, 12))[:, :n_long]
    x1 = helpers.synth_stream(502, n_short)
    one = lamehip.Batch(enc, 2, n_long + 16)
    one.set_pcm(0, x0[0], x0[1])
    one.set_pcm(1, x1[0], x1[1])
    one.encode()
    want = [one.pack(0), one.pack(1)]
    one.close()
    b = lamehip.Batch(enc, 2, n_long + 16)
    for attempt in range(2):
        b.append(0, np.zeros(0, np.int16), np.zeros(0, np.int16))      # nothing, as the very first call
        b.append(0, x0[0], x0[1])                                       # 2.6 M samples at once
        out = [b"", b""]
        for at in range(0, n_short, 5000):                              # small chunks of the other stream, encoded as they come
            b.append(1, x1[0, at:at + 5000], x1[1, at:at + 5000])
            b.encode_available()
            for s in range(2):
                out[s] += b.drain(s, 1 << 24)
        b.finish()
        for s in range(2):
            out[s] += b.drain(s, 1 << 24)
        assert out == want, attempt
        for call in (lambda: b.append(1, x1[0, :10], x1[1, :10]), b.encode_available, b.finish, b.encode):
            with pytest.raises(RuntimeError):
                call()
        b.reset()
    b.close()
    enc.close()


REGROW_SECONDS = (0.25, 1.5, 0.25)      # per round: the second outgrows what the first allocated, the third fits again


def _regrow_streams(rate, rnd):
    n = int(rate * REGROW_SECONDS[rnd])
    return [helpers.synth_stream(9100 + 10 * rnd + i, k, rate) for i, k in enumerate((n, n - 777, n // 2))]


def _device_packed_batch(enc, nstreams, cap, resample):
    b = lamehip.Batch(enc, nstreams, cap)
    b.set_device_packing()
    if resample:
        b.set_device_resampling()
    return b


def _encode_and_fetch(b, pcms):
    """through the pinned mirror, asynchronously, and back through the pinned byte buffer"""
    h = b.pcm_host()
    for s, x in enumerate(pcms):
        h[s, :, :x.shape[1]] = x
        b.set_length(s, x.shape[1])
        b.mark_pcm(s)
    b.encode(sync=False)
    b.fetch()
    return [bytes(b.bytes_view(s)) for s in range(len(pcms))]


@functools.lru_cache(maxsize=None)
def _regrow_reference(rate):
    """per round: the bytes of a fresh batch given that round's streams (computed once per input rate)"""
    enc = lamehip.Encoder(rate, out_samplerate=44100, brate=128)
    want = []
    for rnd in range(len(REGROW_SECONDS)):
        f = _device_packed_batch(enc, 3, 2 * rate, rate != 44100)
        want.append(_encode_and_fetch(f, _regrow_streams(rate, rnd)))
        f.close()
    enc.close()
    return want


def _lifecycle_bytes(kind):
    """one batch of `kind' from creation to close: its streams' bytes"""
    rate = 48000 if kind == "device-resampling" else 44100
    pcms = [helpers.synth_stream(9200 + i, rate // 2 - 333 * i, rate) for i in range(2)]
    enc = lamehip.Encoder(rate, out_samplerate=44100, brate=128)
    if kind == "pipelined":
        b = _device_packed_batch(enc, 2, rate // 2, False)
        out = _encode_and_fetch(b, pcms)
    elif kind == "incremental":
        b = lamehip.Batch(enc, 2, rate // 2)
        out = [b"", b""]
        for at in range(0, rate // 2, 1000):
            for s, x in enumerate(pcms):
                b.append(s, x[0, at:at + 1000], x[1, at:at + 1000])
            b.encode_available()
            for s in range(2):
                out[s] += b.drain(s)
        b.finish()
        for s in range(2):
            out[s] += b.drain(s)
    else:
        b = lamehip.Batch(enc, 2, rate // 2)
        if kind == "device-resampling":
            b.set_device_resampling()
        for s, x in enumerate(pcms):
            b.set_pcm(s, x[0], x[1])
        b.encode()
        out = [b.pack(s) for s in range(2)]
    b.close()
    enc.close()
    assert all(len(x) > 0 for x in out), kind
    return out


@pytest.mark.gpu
def test_batch_buffers_regrow_on_a_live_batch_and_lifecycles_repeat(monkeypatch):
    """What the batch's resource handling can get wrong without any kernel being involved.

    Regrow: one device-packed batch of 3 streams (capacity 2 s) through rounds of 0.25 s, 1.5 s and 0.25 s streams -- the
    second round outgrows the payload pool, the byte pool, its pinned mirror and the analysis pool of a batch that has
    work behind it.  Every round's bytes equal a fresh batch's and the host packer's from the same frames.  The same for
    a 48 -> 44.1 kHz batch that converts on the device (the conversion plan's buffers grow behind the stream's work) and
    for launches in windows of 3 frames (the windows' descriptors and events grow).

    Lifecycle: create, use, close, three times over, for a plain, a pipelined device-packed, a device-resampling and an
    incremental batch: identical bytes every time, and lamehip_last_error() stays empty."""
    for rate, window in ((44100, None), (48000, None), (44100, "3")):
        if window:
            monkeypatch.setenv("LAMEHIP_MID_WINDOW", window)
        want = _regrow_reference(44100 if window else rate)
        enc = lamehip.Encoder(rate, out_samplerate=44100, brate=128)
        b = _device_packed_batch(enc, 3, 2 * rate, rate != 44100)
        for rnd in range(len(REGROW_SECONDS)):
            got = _encode_and_fetch(b, _regrow_streams(rate, rnd))
            assert b.windows() == (1 if not window else -(-max(b.frames(s) for s in range(3)) // 3)), (rate, window, rnd)
            for s in range(3):
                assert got[s] == want[rnd][s], (rate, window, rnd, s, "fresh batch")
                assert got[s] == b.pack(s), (rate, window, rnd, s, "host packer")
        b.close()
        enc.close()
        monkeypatch.delenv("LAMEHIP_MID_WINDOW", raising=False)
    for kind in ("plain", "pipelined", "device-resampling", "incremental"):
        cycles = []
        for _ in range(3):
            cycles.append(_lifecycle_bytes(kind))
            assert lamehip.last_error() == "", (kind, lamehip.last_error())
        assert cycles[0] == cycles[1] == cycles[2], kind
