"""The tag frames of a device-packed batch without a device: the SOURCE of the tag kernel (csrc/lh_tag.hip) run by the
fiber emulator of tests/hipemu against the host's bookkeeping (csrc/lh_vbrtag.c: lh_tag_crc, lh_tag_add_frame,
lh_tag_frame) byte for byte -- and, where the compiled reference is there, against its lame_get_lametag_frame --; the gain
patch against lh_tag_frame with the gain; and the host side as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import lamehip

TAG_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_tag")
PIECE, WAVE, ROW = 16, 64 * 16, 256 * 16     # LH_TAG_PIECE, a wave's pieces, LH_TAG_ROW (csrc/lh_tag.h)


class LhVbrTag(C.Structure):
    _fields_ = [("enabled", C.c_int), ("total_frame_size", C.c_int), ("sum", C.c_int), ("seen", C.c_int),
                ("want", C.c_int), ("pos", C.c_int), ("size", C.c_int), ("bag", C.c_int * 400),
                ("num_frames", C.c_uint), ("bytes_written", C.c_ulong), ("music_crc", C.c_uint16), ("samplerate_in", C.c_int),
                ("radio_gain_on", C.c_int), ("radio_gain", C.c_int), ("nogap_total", C.c_int), ("nogap_current", C.c_int)]


class LhTagParams(C.Structure):
    _fields_ = [("total", C.c_int), ("at", C.c_int), ("sideinfo_len", C.c_int), ("error_protection", C.c_int),
                ("kbps", C.c_int16 * 16), ("adv", (C.c_uint16 * 16) * 8)]


# name, Encoder keywords
CONFIGS = [("cbr128-48k", dict(samplerate=48000, brate=128)), ("cbr320-48k", dict(samplerate=48000, brate=320)),
           ("V2", dict(vbr_q=2)), ("abr150", dict(abr=150)), ("vbr-old-V3", dict(vbr_q=3, vbr_mode=2)),
           ("cbr64-22k", dict(samplerate=22050, brate=64)), ("cbr32-12k", dict(samplerate=12000, brate=32)),
           ("mono", dict(brate=128, channels=1)), ("crc-cbr160", dict(brate=160, error_protection=True)),
           ("crc-V4", dict(vbr_q=4, error_protection=True))]


@pytest.fixture(scope="module")
def lib():
    lib = lamehip.load_library()
    lib.lh_tag_crc.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.lh_tag_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    lib.lh_tag_template.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.lh_tag_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_tag.so"], TAG_DIR)
    e = C.CDLL(os.path.join(TAG_DIR, "libhipemu_tag.so"))
    e.lh_emu_tag_crc.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    e.lh_emu_tag_bag.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    e.lh_emu_tag.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 9
    return e


def settings(lib, kw):
    """(encoder, its config, a fresh LhVbrTag, the kernel's parameters, the template) of one row of CONFIGS"""
    enc = lamehip.Encoder(require_device=False, **kw)
    cfg = enc.config()
    v = LhVbrTag()
    total = lib.lh_tag_init(C.byref(v), C.byref(cfg))
    assert total > 0
    p = LhTagParams()
    lib.lh_tag_params(C.byref(v), C.byref(cfg), C.byref(p))
    assert p.total == total
    tmpl = C.create_string_buffer(total)
    lib.lh_tag_template(C.byref(v), C.byref(cfg), cfg.vbr_q, tmpl)
    return enc, cfg, v, p, tmpl.raw


def host_crc(lib, data):
    v = LhVbrTag()
    lib.lh_tag_crc(C.byref(v), bytes(data), len(data))
    return v.music_crc


@pytest.fixture(scope="module")
def params(lib):
    enc, cfg, v, p, tmpl = settings(lib, dict(brate=128))
    enc.close()
    return p


CRC_LENGTHS = ([0, 1, 15, 16, 17, WAVE - 1, WAVE, WAVE + 1, ROW - 1, ROW, ROW + 1, 2 * ROW - 1, 2 * ROW + 1]
               + [int(x) for x in np.random.default_rng(99).integers(ROW, 200 * 1024, 3)])


@pytest.mark.parametrize("offset", [0, 1, 7, 2881])
def test_crc_kernel_matches_host_crc(offset, lib, emu, params):
    """the music CRC of random bytes, every length at which the kernel takes another path -- under a piece, a piece, a
    wave's pieces and a workgroup's row each less one, exact and plus one, a few rows --, the slice `offset' bytes behind a
    16-byte boundary.  The bytes around the slice are canaries, none of them zero: a read outside the slice changes the
    result, and a write shows."""
    rng = np.random.default_rng(1000 + offset)
    guard = 4096
    for n in CRC_LENGTHS:
        raw = np.empty(guard + offset + n + guard + 16, np.uint8)
        lead = (-raw.ctypes.data) % 16          # (the slice's place counts from a 16-byte boundary of memory)
        buf = raw[lead:]
        buf[:] = rng.integers(1, 256, len(buf), dtype=np.uint8)
        at = guard + offset
        data = rng.integers(0, 256, n, dtype=np.uint8)
        buf[at:at + n] = data
        before = buf.copy()
        got = C.c_uint(0xdead)
        assert (buf.ctypes.data + at) % 16 == offset % 16
        assert emu.lh_emu_tag_crc(C.byref(params), buf.ctypes.data + at, n, C.byref(got)) == 0
        assert got.value == host_crc(lib, data), (offset, n)
        assert (buf == before).all(), (offset, n)


@pytest.mark.parametrize("n", [0, 1, 2, 399, 400, 401, 799, 800, 801, 1700])
def test_bookkeeping_matches_add_frame(n, lib, emu, params):
    """the bag in closed form against lh_tag_add_frame called n times with random bit rates: its fill, the sampling
    distance, the sum and every sample (the bag halves at 400 frames and again at 800)"""
    rng = np.random.default_rng(n)
    idx = rng.integers(1, 15, max(n, 1)).astype(np.int8)
    v = LhVbrTag()
    v.want, v.size = 1, 400             # (lh_tag_init's)
    for f in range(n):
        lib.lh_tag_add_frame(C.byref(v), int(params.kbps[int(idx[f])]))
    bag = np.full(400, -7, np.int32)
    psw = np.full(3, -7, np.int32)
    assert emu.lh_emu_tag_bag(C.byref(params), idx.ctypes.data, n, bag.ctypes.data, psw.ctypes.data) == 0
    assert list(psw) == [v.pos, v.want, v.sum]
    assert list(bag[:v.pos]) == list(v.bag[:v.pos])
    assert (bag[v.pos:] == -7).all()
    if n in (400, 800):
        assert v.pos == 200 and v.want == n // 200


def run_kernel(emu, p, tmpl, streams, gap=37):
    """lh_tag_kernel under the emulator over `streams' [(audio bytes, status, bit-rate indices, padding, last mode_ext)]:
    the pool starts as 0xA5, the slices lie `gap' bytes apart (so that they are not aligned); returns every stream's tag
    room and checks that nothing but the tag rooms changed"""
    T, B = p.total, len(streams)
    base, cap, at = [], [], 5
    for (audio, status, idx, pad, ext) in streams:
        at += T
        base.append(at)
        cap.append(len(audio) + 11)
        at += len(audio) + 11 + gap
    pool = np.full(at + 64, 0xA5, np.uint8)
    for s, (audio, status, idx, pad, ext) in enumerate(streams):
        pool[base[s]:base[s] + len(audio)] = np.frombuffer(audio, np.uint8)
    before = pool.copy()
    arr = lambda t, x: np.ascontiguousarray(np.array(x, dtype=t))
    nbytes, status = arr(np.int64, [len(x[0]) for x in streams]), arr(np.int32, [x[1] for x in streams])
    nframes, padding = arr(np.int32, [len(x[2]) for x in streams]), arr(np.int32, [x[3] for x in streams])
    ext = arr(np.int32, [x[4] for x in streams])
    idx = arr(np.int8, [i for x in streams for i in x[2]] + [0])
    base_a, cap_a = arr(np.int64, base), arr(np.int64, cap)
    assert emu.lh_emu_tag(C.byref(p), tmpl, B, nbytes.ctypes.data, status.ctypes.data, nframes.ctypes.data, padding.ctypes.data,
                          ext.ctypes.data, idx.ctypes.data, base_a.ctypes.data, cap_a.ctypes.data, pool.ctypes.data) == 0
    tags = []
    for s in range(B):
        tags.append(bytes(pool[base[s] - T:base[s]]))
        pool[base[s] - T:base[s]] = 0xA5
    assert (pool == before).all(), "the kernel wrote outside the tag rooms"
    return tags


def host_frame(lib, cfg, v0, audio, idx, pad, ext, gain=None):
    """lh_tag_frame over the same inputs; None: no frame"""
    v = LhVbrTag.from_buffer_copy(v0)
    for i in idx:
        lib.lh_tag_add_frame(C.byref(v), lib.lh_tag_kbps(cfg.version, int(i)))
    lib.lh_tag_crc(C.byref(v), audio, len(audio))
    if gain is not None:
        v.radio_gain_on, v.radio_gain = 1, gain
    out = C.create_string_buffer(v.total_frame_size)
    k = lib.lh_tag_frame(C.byref(v), C.byref(cfg), cfg.vbr_q, pad, ext, out, len(out))
    return out.raw if k == v.total_frame_size else None


@pytest.mark.parametrize("name,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_kernel_frame_matches_lh_tag_frame(name, kw, lib, emu):
    """the whole kernel over streams of 1, 2, 401 and 1700 frames with random bit rates of the setting's range and random
    bytes: every tag room holds lh_tag_frame's frame; a stream without frames, and one whose packer reported a status, get
    zeros; nothing else in the pool changes"""
    enc, cfg, v0, p, tmpl = settings(lib, kw)
    rng = np.random.default_rng(len(name) * 131 + p.total)
    lo, hi = (cfg.bitrate_index,) * 2 if cfg.vbr == 0 else (cfg.vbr_min_bitrate_index, cfg.vbr_max_bitrate_index)
    streams = []
    for s, nf in enumerate([1, 0, 2, 401, 7, 1700]):
        audio = rng.integers(0, 256, 0 if nf == 0 else int(rng.integers(1, 9000)) + 16 * s, dtype=np.uint8).tobytes()
        idx = [int(i) for i in rng.integers(lo, hi + 1, nf)]
        streams.append((audio, 3 if nf == 7 else 0, idx, int(rng.integers(0, 2400)), int(rng.integers(0, 4))))
    tags = run_kernel(emu, p, tmpl, streams)
    for s, (audio, status, idx, pad, ext) in enumerate(streams):
        want = host_frame(lib, cfg, v0, audio, idx, pad, ext)
        if status or not idx:
            assert want is None or status
            assert tags[s] == bytes(p.total), (name, s)
        else:
            assert tags[s] == want, (name, s)
    enc.close()


REF_CONFIGS = [c for c in CONFIGS]


@pytest.mark.skipif(not helpers.have_reference(), reason="needs oracle/_ref (reference sources)")
@pytest.mark.parametrize("name,kw", REF_CONFIGS, ids=[c[0] for c in REF_CONFIGS])
def test_kernel_frame_matches_reference(name, kw, lib, emu):
    """the reference's own audio bytes and the oracle's frames through the kernel: the tag room holds the reference's
    final tag frame (as tests/test_lametag.py checks of lh_tag_frame)"""
    sr = kw.get("samplerate", 44100)
    n = int(sr * 0.8)
    nch = kw.get("channels", 2)
    pcm = helpers.synth_stream(4243, n, sr, 1.0 / 5)
    if nch == 1:
        pcm = np.stack([pcm[0], pcm[0]])
    ref = helpers.Reference()
    ref.lib.refh_option.argtypes = [C.c_char_p, C.c_float]
    ref.lib.refh_option(None, 0)
    if kw.get("error_protection"):
        ref.lib.refh_option(b"error_protection", 1.0)
    try:
        stream, tag = helpers.reference_tagged(pcm, sr, kw.get("brate", 0), vbr_q=kw.get("vbr_q"), abr=kw.get("abr"), channels=nch,
                                               vbr_mode=kw.get("vbr_mode", 4))
    finally:
        ref.lib.refh_option(None, 0)
    enc, cfg, v0, p, tmpl = settings(lib, kw)
    assert p.total == len(tag)
    fr = helpers.Oracle().encode_frames(cfg, enc.tables(), pcm)
    audio = stream[len(tag):]
    pad = lib.lh_end_padding_fs(C.c_long(n), 576 * cfg.mode_gr)
    tags = run_kernel(emu, p, tmpl, [(audio, 0, [int(f.bitrate_index) for f in fr], pad, int(fr[-1].mode_ext))])
    assert tags[0] == tag
    enc.close()


@pytest.mark.parametrize("name,kw", [CONFIGS[0], CONFIGS[2], CONFIGS[8]], ids=[CONFIGS[i][0] for i in (0, 2, 8)])
def test_gain_patch_equals_frame_with_gain(name, kw, lib, emu):
    """a frame the kernel made with the gain field zero, patched on the host (lh_tag_patch_gain, through the emulator
    library's copy of csrc/lh_tag.h), is lh_tag_frame's frame with radio_gain_on and that gain"""
    enc, cfg, v0, p, tmpl = settings(lib, kw)
    rng = np.random.default_rng(5)
    audio = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    lo, hi = (cfg.bitrate_index,) * 2 if cfg.vbr == 0 else (cfg.vbr_min_bitrate_index, cfg.vbr_max_bitrate_index)
    idx = [int(i) for i in rng.integers(lo, hi + 1, 12)]
    made = run_kernel(emu, p, tmpl, [(audio, 0, idx, 1105, 2)])[0]
    assert made == host_frame(lib, cfg, v0, audio, idx, 1105, 2)
    emu.lh_emu_tag_patch_gain.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for g in (-0x1FF, -1, 0, 1, 64, 0x1FF):
        buf = C.create_string_buffer(made, len(made))
        emu.lh_emu_tag_patch_gain(buf, p.at, g)
        assert buf.raw == host_frame(lib, cfg, v0, audio, idx, 1105, 2, gain=g), g
    enc.close()


def test_host_side_under_sanitizers():
    """the stand-alone program (its own main; AddressSanitizer and UBSan linked in): template, finish and gain patch over
    every setting and frame count, the kernel's advance matrices against the table CRC"""
    helpers.locked_make(["tag_host_check"], TAG_DIR)
    r = subprocess.run([os.path.join(TAG_DIR, "tag_host_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
    assert "FAILED" not in r.stdout


def test_symbols_are_declared_and_exported():
    lib = lamehip.load_library()
    txt = open(os.path.join(helpers.ROOT, "include", "lamehip.h")).read()
    for name in ("lamehip_batch_set_device_tagging", "lamehip_batch_image_ptr", "lamehip_batch_get_images_all",
                 "lamehip_batch_last_tag_ms"):
        assert name + "(" in txt and hasattr(lib, name), name
    for name in ("lh_launch_tag", "lh_tag_template", "lh_tag_params", "lh_tag_frame"):
        assert hasattr(lib, name), name
    for name in ("set_device_tagging", "image", "images_all", "tag_ms"):
        assert hasattr(lamehip.Batch, name), name
