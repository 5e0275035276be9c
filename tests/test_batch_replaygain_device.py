"""A batch's ReplayGain on the device (lamehip_batch_set_replaygain, csrc/lh_gain.hip): the window sums the kernel leaves
are the host twin's bit for bit on what the batch's encoder reads, the gain is lame_get_RadioGain of a handle fed the same
stream a frame's worth per call and flushed, the tagged outputs are the handle's file image, and nothing changes while the
switch is off."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gain_support as gs
import helpers
import lamehip

pytestmark = pytest.mark.gpu

IDS = [s[0] for s in gs.SETTINGS]


def streams_of(k):
    """the ragged batch of setting k: the list of lengths, amplitudes alternating 1 and 0.25, and last a 0.5 s stream followed
    by 0.3 s of digital silence"""
    setting = gs.SETTINGS[k]
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    xs = [gs.signal(setting, 9100 + 20 * k + s, n, 1.0 if s % 2 == 0 else 0.25)
          for s, n in enumerate(gs.lengths_of(rate_in, rate_out, fs))]
    quiet = gs.signal(setting, 9119 + 20 * k, int(0.8 * rate_in))
    quiet[:, int(0.5 * rate_in):] = 0
    return xs + [quiet]


@functools.lru_cache(maxsize=None)
def handle_gains(k):
    """per setting, computed once: lame_get_RadioGain of every stream of streams_of(k)"""
    setting = gs.SETTINGS[k]
    gains = []
    for x in streams_of(k):
        enc = gs.open_handle(setting, find_gain=True)
        gains.append(gs.handle_stream(enc, setting, x)[1])
        enc.close()
    return gains


def check_streams(lib, b, enc, setting, xs, want_gains, what=""):
    """every stream: windows bit-equal to the host twin, gain equal to the twin's and to the handle's; returns the windows"""
    wins = []
    for s, x in enumerate(xs):
        pairs, tenths = gs.expected_of_stream(lib, b, enc, setting, s, x)
        got = b.gain_windows(s)
        assert gs.same_doubles(got, pairs), "%s stream %d (%d samples): window sums" % (what, s, x.shape[1])
        assert b.radio_gain(s) == tenths, "%s stream %d: gain against the host twin" % (what, s)
        assert b.radio_gain(s) == want_gains[s], "%s stream %d: gain against the handle" % (what, s)
        wins.append(got)
    return wins


@pytest.mark.parametrize("k", range(len(gs.SETTINGS)), ids=IDS)
def test_ragged_batch_matches_host_twin_and_handle(k):
    setting = gs.SETTINGS[k]
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    lib = gs.library()
    xs = streams_of(k)
    cap = max(x.shape[1] for x in xs) + 3
    enc = gs.open_handle(setting)
    b = gs.make_batch(enc, setting, len(xs), cap)
    b.set_replaygain()
    if stype == "f32unit":
        gs.feed_batch_in_place(b, setting, xs, cap)     # device-resident: the pool itself, NaN beyond every length
    else:
        gs.feed_batch(b, setting, xs)
    b.encode()
    assert b.gain_ms() > 0.0
    # first: the last stream ends in silence, and a late window of the host twin is a sum of squares of subnormals -- so the
    # comparison below covers such a window
    late = gs.expected_of_stream(lib, b, enc, setting, len(xs) - 1, xs[-1])[0][-1]
    assert 0 < late[0] + late[1] < 1e-70
    wins = check_streams(lib, b, enc, setting, xs, handle_gains(k), name)
    assert gs.same_doubles(wins[-1][-1:], late.reshape(1, 2))
    gains = [b.radio_gain(s) for s in range(len(xs))]
    assert len(set(gains) - {0}) >= 2
    if channels == 1:
        assert all((w[:, 0] == w[:, 1]).all() for w in wins)
    b.close()
    enc.close()


@pytest.mark.parametrize("nstreams", [383, 384])
def test_either_side_of_the_mapping_threshold(nstreams):
    """LH_GN_TAPS_BELOW = 384 streams in a launch: below it the first filter's feedback runs across the lanes of a row, from it
    on in lanes 0 and 1; short streams, the first, the last and two in between against the host twin"""
    setting = gs.SETTINGS[0]
    lib = gs.library()
    base = [gs.signal(setting, 9900 + s, 2700 - 11 * s, 1.0 if s % 2 == 0 else 0.25) for s in range(4)]
    enc = gs.open_handle(setting)
    b = gs.make_batch(enc, setting, nstreams, 2700)
    b.set_replaygain()
    gs.feed_batch(b, setting, [base[s % 4] for s in range(nstreams)])
    b.encode()
    for s in (0, 129, 254, nstreams - 1):
        pairs, tenths = gs.expected_of_stream(lib, b, enc, setting, s, base[s % 4])
        assert len(pairs) >= 1 and gs.same_doubles(b.gain_windows(s), pairs) and b.radio_gain(s) == tenths != 0, s
    b.close()
    enc.close()


@pytest.mark.parametrize("forced", ["0", "1"], ids=["taps-across-lanes", "lanes-0-and-1"])
def test_mapping_forced(forced, monkeypatch):
    """LAMEHIP_GAIN_LANES=0 / 1 (the measurement aid of tools/replaygain_bench.py): either mapping whatever the launch's size,
    the same sums"""
    monkeypatch.setenv("LAMEHIP_GAIN_LANES", forced)
    k = 0
    setting = gs.SETTINGS[k]
    xs = streams_of(k)
    enc = gs.open_handle(setting)
    b = gs.make_batch(enc, setting, len(xs), max(x.shape[1] for x in xs))
    b.set_replaygain()
    gs.feed_batch(b, setting, xs)
    b.encode()
    check_streams(gs.library(), b, enc, setting, xs, handle_gains(k), "LAMEHIP_GAIN_LANES=%s," % forced)
    b.close()
    enc.close()


def test_batch_that_converts_on_the_host():
    """44.1 -> 32 kHz without device resampling: set_pcm converts on the host, the analysis hears the float planes in the blocks
    of that conversion's plan"""
    k = 6
    setting = gs.SETTINGS[k]
    xs = streams_of(k)
    enc = gs.open_handle(setting)
    b = lamehip.Batch(enc, len(xs), max(x.shape[1] for x in xs))
    b.set_replaygain()
    gs.feed_batch(b, setting, xs)
    b.encode()
    assert b.gain_ms() > 0.0 and b.resample_ms() == 0.0
    check_streams(gs.library(), b, enc, setting, xs, handle_gains(k), "host conversion,")
    b.close()
    enc.close()


def test_many_streams_in_one_launch():
    """67 streams of 0.2 s: several workgroups, more streams than a wave has lanes, the last workgroup not full"""
    setting = gs.SETTINGS[0]
    lib = gs.library()
    n = int(0.2 * 44100)
    xs = [gs.signal(setting, 9400 + s, n - 3 * s, 1.0 if s % 2 == 0 else 0.25) for s in range(67)]
    want = []
    for x in xs:
        h = gs.open_handle(setting, find_gain=True)
        want.append(gs.handle_stream(h, setting, x)[1])
        h.close()
    enc = gs.open_handle(setting)
    b = gs.make_batch(enc, setting, len(xs), n + 1)
    b.set_replaygain()
    gs.feed_batch(b, setting, xs)
    b.encode()
    check_streams(lib, b, enc, setting, xs, want, "67 streams,")
    assert len(set(want) - {0}) >= 2
    b.close()
    enc.close()


@pytest.mark.parametrize("k", [0, 5], ids=[IDS[0], IDS[5]])
def test_pool_poisoned_beyond_every_length(k):
    """the pool written through pcm_device_ptr with 0x7fff / NaN at and beyond every stream's length: the results of the
    batch fed from host arrays"""
    setting = gs.SETTINGS[k]
    xs = streams_of(k)
    cap = max(x.shape[1] for x in xs) + 5
    enc = gs.open_handle(setting)
    res = []
    for in_place in (False, True):
        b = gs.make_batch(enc, setting, len(xs), cap)
        b.set_replaygain()
        if in_place:
            gs.feed_batch_in_place(b, setting, xs, cap)
        else:
            gs.feed_batch(b, setting, xs)
        b.encode()
        res.append([(b.gain_windows(s).tobytes(), b.radio_gain(s)) for s in range(len(xs))])
        b.close()
    enc.close()
    assert res[0] == res[1]
    assert res[0][-1][1] == handle_gains(k)[-1]


def handle_file_image(setting, x, vbr_q, find_gain):
    """what the frontend leaves on disk: the handle's stream with lame_get_lametag_frame over the placeholder"""
    enc = gs.open_handle(setting, find_gain=find_gain, write_tag=True, vbr_q=vbr_q)
    stream, gain = gs.handle_stream(enc, setting, x)
    tag = enc.lametag_frame()
    enc.close()
    assert len(tag) > 0
    return tag + stream[len(tag):], len(tag), gain


@pytest.mark.parametrize("vbr_q", [None, 2], ids=["cbr128", "V2"])
def test_tagged_outputs_carry_the_gain(vbr_q):
    setting = gs.SETTINGS[0]
    xs = [gs.signal(setting, 9500, int(0.9 * 44100)), gs.signal(setting, 9501, int(0.6 * 44100), 0.25)]
    enc = gs.open_handle(setting, write_tag=True, vbr_q=vbr_q)
    images = {}
    for on in (False, True):
        b = gs.make_batch(enc, setting, len(xs), max(x.shape[1] for x in xs), packing=True)
        if on:
            b.set_replaygain()
        gs.feed_batch(b, setting, xs)
        b.encode()
        for s, x in enumerate(xs):
            want, ntag, gain = handle_file_image(setting, x, vbr_q, on)
            assert gain != 0 if on else gain == 0
            assert b.pack_tagged(s) == want, (on, s)
            assert b.get_bytes_tagged(s) == want, (on, s)
            images[(on, s)] = (want, ntag)
        b.close()
    enc.close()
    for s in range(len(xs)):
        (off, ntag), (on, ntag_on) = images[(False, s)], images[(True, s)]
        assert ntag == ntag_on and off[ntag:] == on[ntag:] and off[:ntag] != on[:ntag]
    assert images[(True, 0)][0][:images[(True, 0)][1]] != images[(True, 1)][0][:images[(True, 1)][1]]


def test_frame_windows_one_analysis():
    """LAMEHIP_MID_WINDOW=64, two streams of about 4 s, in a process of its own (tests/gain_window_child.py): the launch runs
    in windows of frames, the analysis ran (gain_ms() > 0) and its windows and gains are those of the whole streams.  (That it
    is launched once, outside the loop over the frame windows, is lamehip_batch_encode's structure: a time cannot show it.)"""
    child = os.path.join(helpers.ROOT, "tests", "gain_window_child.py")
    env = dict(os.environ, LAMEHIP_MID_WINDOW="64")
    r = subprocess.run([sys.executable, child], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "gain under frame windows ok" in r.stdout, r.stdout[-3000:]


def test_redeclaration_and_reset():
    setting = gs.SETTINGS[0]
    lib = gs.library()
    xs = [gs.signal(setting, 9600, 30000), gs.signal(setting, 9601, 20000, 0.25)]
    other = gs.signal(setting, 9602, 25000, 0.05)
    enc = gs.open_handle(setting)
    b = gs.make_batch(enc, setting, 2, 30000)
    b.set_replaygain()
    gs.feed_batch(b, setting, xs)
    b.encode()
    first = [(b.gain_windows(s).tobytes(), b.radio_gain(s)) for s in range(2)]
    want_other = gs.eval_host(lib, 44100, 2, gs.plan(lib, None, 1152, 25000)[0], gs.heard_by_batch(b, enc, setting, 1, other))
    b.set_pcm(1, other[0], other[1])
    b.encode()
    assert b.gain_ms() > 0.0
    assert (b.gain_windows(0).tobytes(), b.radio_gain(0)) == first[0]
    assert gs.same_doubles(b.gain_windows(1), want_other[0]) and b.radio_gain(1) == want_other[1] != first[1][1]
    # nothing declared: nothing analysed, every result kept
    b.encode()
    assert b.gain_ms() == 0.0
    assert b.radio_gain(1) == want_other[1] and (b.gain_windows(0).tobytes(), b.radio_gain(0)) == first[0]
    # reset: no result until the next encode, which measures every stream again
    b.reset()
    v = C.c_int(7)
    b.lib.lamehip_batch_radio_gain.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    assert b.lib.lamehip_batch_radio_gain(b.b, 0, C.byref(v)) == -1 and v.value == 7
    assert b"lamehip_batch_radio_gain" in b.lib.lamehip_last_error()
    b.encode()
    assert b.gain_ms() > 0.0
    assert (b.gain_windows(0).tobytes(), b.radio_gain(0)) == first[0] and b.radio_gain(1) == want_other[1]
    b.close()
    enc.close()


def test_refusals_and_the_switch_off():
    lib = lamehip.load_library()
    lib.lamehip_batch_set_replaygain.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_batch_radio_gain.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.lamehip_batch_get_gain_windows.restype = C.c_long
    lib.lamehip_batch_get_gain_windows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.lamehip_batch_encode_available.argtypes = [C.c_void_p]
    lib.lamehip_batch_finish.argtypes = [C.c_void_p]
    setting = gs.SETTINGS[0]
    x = gs.signal(setting, 9700, 5000)
    v = C.c_int(0)
    # the proto's lame_set_findReplayGain is not inherited: no gain, the bytes of a batch of a handle without it
    enc_on = gs.open_handle(setting, find_gain=True, write_tag=True)
    enc = gs.open_handle(setting, write_tag=True)
    images = []
    for e in (enc_on, enc):
        b = lamehip.Batch(e, 1, 5000)
        b.set_pcm(0, x[0], x[1])
        b.encode()
        assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(v)) == -1
        assert b"lamehip_batch_radio_gain" in lib.lamehip_last_error() and b"lamehip_batch_set_replaygain" in lib.lamehip_last_error()
        assert lib.lamehip_batch_get_gain_windows(b.b, 0, None, 0) == -1
        assert b.gain_ms() == 0.0
        images.append(b.pack_tagged(0))
        b.close()
    assert images[0] == images[1]
    # before an encode with the switch on
    b = lamehip.Batch(enc, 1, 5000)
    assert lib.lamehip_batch_set_replaygain(b.b, 1) == 0
    b.set_pcm(0, x[0], x[1])
    assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(v)) == -1
    # incremental calls once it is on, each named
    assert lib.lamehip_batch_append(b.b, 0, x[0].ctypes.data, x[1].ctypes.data, 1000) == -1
    assert b"lamehip_batch_append" in lib.lamehip_last_error() and b"ReplayGain" in lib.lamehip_last_error()
    assert lib.lamehip_batch_encode_available(b.b) == -1
    assert b"lamehip_batch_encode_available" in lib.lamehip_last_error() and b"ReplayGain" in lib.lamehip_last_error()
    assert lib.lamehip_batch_finish(b.b) == -1
    assert b"lamehip_batch_finish" in lib.lamehip_last_error() and b"ReplayGain" in lib.lamehip_last_error()
    b.encode()
    assert lib.lamehip_batch_radio_gain(b.b, 0, C.byref(v)) == 0 and v.value != 0
    assert lib.lamehip_batch_radio_gain(b.b, 1, C.byref(v)) == -1       # no such stream
    b.close()
    # an incremental batch refuses the switch
    b = lamehip.Batch(enc, 1, 5000)
    assert lib.lamehip_batch_append(b.b, 0, x[0].ctypes.data, x[1].ctypes.data, 1000) == 0
    assert lib.lamehip_batch_set_replaygain(b.b, 1) == -1
    assert b"lamehip_batch_set_replaygain" in lib.lamehip_last_error() and b"incremental" in lib.lamehip_last_error()
    b.close()
    enc.close()
    enc_on.close()
