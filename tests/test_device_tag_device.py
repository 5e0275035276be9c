"""Device tagging (lamehip_batch_set_device_tagging) on the GPU: the file images a device-packed batch brings home -- the
tag frame csrc/lh_tag.hip wrote in front of every stream's bytes, then the bytes -- against the host's images of a second
batch without the switch (pack_tagged), against get_bytes_tagged of the same batch and, where the compiled reference is
there, against the file its frontend leaves on disk; the audio getters unchanged; ReplayGain, pipelined use, a second
launch, the switch taken back, what is refused, and a poisoned byte pool."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
import lamehip

pytestmark = pytest.mark.gpu


def open_batch(enc, pcms, tagging=True, gain=False, resample=False, cap=None):
    b = lamehip.Batch(enc, len(pcms), cap or max(max(x.shape[1] for x in pcms), 1))
    b.set_device_packing()
    if resample:
        b.set_device_resampling()
    if tagging:
        b.set_device_tagging()
    if gain:
        b.set_replaygain()
    for s, x in enumerate(pcms):
        b.set_pcm(s, x[0], x[1])
    return b


def images_of(b, n):
    """every stream's image three ways -- in place, all at once, copied from HBM --, which must agree"""
    b.fetch()
    out, sizes = b.images_all()
    res = []
    for s in range(n):
        img = bytes(b.image(s))
        assert img == bytes(out[s, :sizes[s]]), s
        assert img == b.get_bytes_tagged(s), s
        res.append(img)
    return res


def check_against_plain(enc, pcms, what, gain=False, resample=False, reference=None):
    """the switched batch's images == pack_tagged of a batch without the switch (== the reference's file, where given);
    its audio getters == the plain batch's"""
    tagged = open_batch(enc, pcms, True, gain, resample)
    plain = open_batch(enc, pcms, False, gain, resample)
    tagged.encode()
    plain.encode()
    imgs = images_of(tagged, len(pcms))
    assert tagged.tag_ms() > 0 and plain.tag_ms() == 0
    all_t, sizes_t = tagged.get_bytes_all()
    all_p, sizes_p = plain.get_bytes_all()
    assert list(sizes_t) == list(sizes_p)
    for s in range(len(pcms)):
        assert imgs[s] == plain.pack_tagged(s), (what, s)
        assert imgs[s] == plain.get_bytes_tagged(s), (what, s)
        if reference is not None:
            assert imgs[s] == reference[s], (what, s)
        audio = plain.get_bytes(s)
        assert tagged.get_bytes(s) == audio and bytes(tagged.bytes_view(s)) == audio, (what, s)
        assert bytes(all_t[s, :sizes_t[s]]) == audio
        assert imgs[s][len(imgs[s]) - len(audio):] == audio
    tagged.close()
    plain.close()
    return imgs


def samples_for_frames(lib, frames):
    """a stream length that gives exactly `frames' frames at 1152 samples per frame"""
    n = max((frames - 3) * 1152, 1)
    while lib.lh_total_frames(C.c_long(n)) < frames:
        n += 1152
    while lib.lh_total_frames(C.c_long(n - 100)) == frames:
        n -= 100                # (near the lower end of the lengths that give this count, and no multiple of anything)
    assert lib.lh_total_frames(C.c_long(n)) == frames
    return n


@functools.lru_cache(maxsize=None)
def ragged_streams():
    lib = lamehip.load_library()
    sr = 44100
    lengths = [0, 1, 1152] + [samples_for_frames(lib, f) for f in (399, 400, 401, 801)] + [int(sr * 0.8)]
    return [helpers.synth_stream(900 + k, n, sr, 1.0 / 4) if n else np.zeros((2, 0), np.int16) for k, n in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def ragged_reference():
    """the reference's file images of the ragged streams (None without the compiled reference; a stream without samples
    has none: the library's own answer is checked instead)"""
    if not helpers.have_reference():
        return None
    res = []
    for x in ragged_streams():
        if x.shape[1] == 0:
            res.append(None)
            continue
        stream, tag = helpers.reference_tagged(x, 44100, 128)
        res.append(tag + stream[len(tag):])
    return res


def test_ragged_batch_images():
    """8 streams at 44.1 kHz CBR 128: no samples, one sample, one frame's worth, 399 / 400 / 401 / 801 frames (the bag fills,
    halves, and halves again) and 0.8 s"""
    pcms = ragged_streams()
    enc = lamehip.Encoder(44100, 128)
    lib = enc.lib
    probe = open_batch(enc, pcms)
    nframes = [probe.frames(s) for s in range(len(pcms))]
    probe.close()
    assert nframes[3:7] == [399, 400, 401, 801]
    ref = ragged_reference()
    imgs = check_against_plain(enc, pcms, "ragged")
    v = C.create_string_buffer(4096)
    total = lib.lh_tag_init(v, C.byref(enc.config()))
    assert total == 417
    for s, nf in enumerate(nframes):
        if nf == 0:     # a stream without frames: the tag room zeroed, no audio
            assert imgs[s] == bytes(total)
        else:
            assert len(imgs[s]) > total and imgs[s][36:40] == b"Info"
    if ref is not None:
        for s, want in enumerate(ref):
            if want is not None:
                assert imgs[s] == want, s
    enc.close()


SETTINGS = [("V2", dict(vbr_q=2), {}), ("abr180", dict(abr=180), {}), ("vbr-old-V3", dict(vbr_q=3, vbr_mode=2), {}),
            ("cbr56-22k", dict(samplerate=22050, brate=56), {}), ("cbr24-12k", dict(samplerate=12000, brate=24), {}),
            ("mono", dict(brate=128, channels=1), {}), ("crc", dict(brate=160, error_protection=True), {}),
            ("resample-48-44", dict(samplerate=48000, out_samplerate=44100, brate=128), dict(resample=True)),
            ("window3", dict(brate=128), dict(window=3))]


@pytest.mark.parametrize("name,kw,how", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_settings_images(name, kw, how, monkeypatch):
    """four short streams per setting: VBR, ABR, the old VBR loop, MPEG-2 and 2.5, mono, error protection, the source
    frequency bits of a batch that converts 48 -> 44.1 kHz on the device, a launch in windows of three frames"""
    sr = kw.get("samplerate", 44100)
    pcms = [helpers.synth_stream(777 + i, int(sr * (0.8 + 0.37 * i)), sr, 1.0 / 4) for i in range(4)]
    if kw.get("channels") == 1:
        pcms = [np.stack([x[0], x[0]]) for x in pcms]
    if "window" in how:
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", str(how["window"]))
    reference = None
    if helpers.have_reference() and name in ("V2", "abr180", "vbr-old-V3", "cbr56-22k", "cbr24-12k", "mono", "window3"):
        reference = []
        for x in pcms:
            stream, tag = helpers.reference_tagged(x, sr, kw.get("brate", 0), vbr_q=kw.get("vbr_q"), abr=kw.get("abr"),
                                                   channels=kw.get("channels", 2), vbr_mode=kw.get("vbr_mode", 4))
            reference.append(tag + stream[len(tag):])
    enc = lamehip.Encoder(**kw)
    imgs = check_against_plain(enc, pcms, name, resample=bool(how.get("resample")), reference=reference)
    if "window" in how:
        b = open_batch(enc, pcms)
        b.encode()
        assert b.windows() > 1
        assert images_of(b, len(pcms)) == imgs
        b.close()
    if name == "crc":
        assert all(img[4:6] != b"\0\0" for img in imgs)
    enc.close()


def test_replaygain_images():
    """ReplayGain on: the image is pack_tagged's with ReplayGain on, and differs from the image without it in the two bytes
    of the gain field and the two of the tag's CRC only"""
    sr = 44100
    pcms = [helpers.synth_stream(300 + i, int(sr * (0.9 + 0.3 * i)), sr, 1.0 / 4) for i in range(4)]
    enc = lamehip.Encoder(sr, 128)
    with_gain = check_against_plain(enc, pcms, "replaygain", gain=True)
    without = check_against_plain(enc, pcms, "no replaygain")
    at = enc.config().sideinfo_len + 116
    for a, b in zip(with_gain, without):
        assert len(a) == len(b)
        differ = [i for i in range(len(a)) if a[i] != b[i]]
        assert differ and set(differ) <= {at + 19, at + 20, at + 38, at + 39}, differ
        assert a[at + 19] & 0x20            # (name code 1: a radio gain)
    enc.close()


def test_pipelined_second_launch_and_switch_off():
    """two batches in flight (encode, fetch, then image_ptr of both); a batch encoded a second time with other, shorter
    streams -- no stale frame in the tag room --; the switch taken back: audio only, and tag_ms() == 0"""
    sr = 44100
    first = [helpers.synth_stream(50 + i, int(sr * (1.0 + 0.2 * i)), sr, 1.0 / 4) for i in range(3)]
    second = [helpers.synth_stream(60 + i, int(sr * (0.5 + 0.1 * i)), sr, 1.0 / 4) for i in range(3)]
    enc = lamehip.Encoder(sr, 128)
    cap = max(x.shape[1] for x in first)
    plain = []
    for pcms in (first, second):
        p = open_batch(enc, pcms, tagging=False, cap=cap)
        p.encode()
        plain.append(([p.pack_tagged(s) for s in range(3)], [p.get_bytes(s) for s in range(3)]))
        p.close()
    a, b = open_batch(enc, first, cap=cap), open_batch(enc, second, cap=cap)
    a.encode(sync=False)
    a.fetch()
    b.encode(sync=False)
    b.fetch()
    assert [bytes(a.image(s)) for s in range(3)] == plain[0][0]
    assert [bytes(b.image(s)) for s in range(3)] == plain[1][0]
    # the same batch again, now with the shorter streams
    for s, x in enumerate(second):
        a.set_pcm(s, x[0], x[1])
    a.encode()
    assert a.tag_ms() > 0
    assert images_of(a, 3) == plain[1][0]
    # and once more with the switch off
    a.set_device_tagging(False)
    a.encode()
    assert a.tag_ms() == 0
    with pytest.raises(RuntimeError, match="lamehip_batch_set_device_tagging"):
        a.image(0)
    assert [bytes(a.bytes_view(s)) for s in range(3)] == plain[1][1]
    assert [a.get_bytes_tagged(s) for s in range(3)] == plain[1][0]        # (the host's walk again)
    a.set_device_tagging(True)
    a.encode()
    assert a.tag_ms() > 0 and images_of(a, 3) == plain[1][0]
    a.close()
    b.close()
    enc.close()


def test_refusals():
    sr = 44100
    x = helpers.synth_stream(5, 4000, sr)
    enc = lamehip.Encoder(sr, 128)
    b = lamehip.Batch(enc, 2, 8000)
    with pytest.raises(RuntimeError, match="lamehip_batch_set_device_packing"):
        b.set_device_tagging()
    b.set_device_packing()
    b.set_device_tagging()
    with pytest.raises(RuntimeError, match="lamehip_batch_set_device_packing"):
        b.append(0, x[0], x[1])
    b.close()
    inc = lamehip.Batch(enc, 2, 8000)
    inc.append(0, x[0], x[1])
    with pytest.raises(RuntimeError, match="incremental.*lamehip_batch_set_device_packing"):
        inc.set_device_tagging()
    inc.close()
    enc.close()


def test_poisoned_byte_pool_changes_nothing():
    """the byte pool filled with 0xA5 before the launch: the images are those of the untouched pool (the stream without
    frames among them: its tag room is written, zeros)"""
    pcms = [ragged_streams()[k] for k in (0, 1, 2, 7)]
    enc = lamehip.Encoder(44100, 128)
    clean = open_batch(enc, pcms)
    clean.encode()
    want = images_of(clean, len(pcms))
    clean.close()
    b = open_batch(enc, pcms)
    b.reserve()
    pool, size = b.bytes_device_ptr()
    assert pool and size > 4 * 417
    b.lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert b.lib.hipMemset(pool, 0xA5, size) == 0
    b.encode()
    assert b.bytes_device_ptr() == (pool, size)
    assert images_of(b, len(pcms)) == want
    if b.frames(0) == 0:
        assert want[0] == bytes(417)
    b.close()
    enc.close()
