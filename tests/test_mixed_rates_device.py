"""Incremental converting batches whose streams arrive at rates of their own (lamehip_batch_set_stream_in_samplerate;
csrc/lh_resample_dev.hip: lh_resample_mixed_tiles_kernel): a pool of nine streams at nine input rates, all to one kind of
MP3, fed round by round in ragged chunks.  Every stream's bytes, frames, tag frame and radio gain are those of a handle with
(in = the stream's rate, out = the batch's output rate given explicitly) fed the same calls -- the compiled reference where
it is built, the library's own handle API else --, and converted(s) is the host chain at the stream's rate; slots that change
their rate, a pool at the batch's own rate, and what is refused."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import lamehip
import mixed_rates_support as msup
import pcm_input_support as psup
import test_append_input_device as taid
import test_append_resample_device as tard
import test_pcm_input_device as t
from lamehip import PCM_S16
from mixed_rates_support import OUT, RATES

pytestmark = pytest.mark.gpu

OWN = 48000                     # the batch's own input rate: class 0
JS128 = dict(brate=128, mode=1)


class Handle:
    """One stream's yardstick: a handle at (in = hz, out given explicitly) with the tag frame on, fed s16 call by call.  The
    compiled reference where it is built -- unless the radio gain is asked for, which its harness has no switch for: then,
    and where it is not built, the library's own handle API."""

    def __init__(self, hz, kw, out=OUT, gain=False):
        self.buf = C.create_string_buffer(400000)
        self.ref = helpers.Reference() if helpers.have_reference() and not gain else None
        if self.ref:
            lib = self.ref.lib
            lib.refh_option.argtypes = [C.c_char_p, C.c_float]
            lib.refh_open_tag.restype = C.c_void_p
            lib.refh_open_vbr.restype = C.c_void_p
            lib.refh_option(None, 0)
            lib.refh_option(b"out_samplerate", float(out))
            lib.refh_set_channels(kw.get("channels", 2))
            try:
                if "vbr_q" in kw:
                    self.h = lib.refh_open_vbr(hz, kw["vbr_q"], kw.get("mode", -1), -1, out, 1)
                else:
                    self.h = lib.refh_open_tag(hz, kw["brate"], kw.get("mode", -1), -1)
            finally:
                lib.refh_option(None, 0)
                lib.refh_set_channels(2)
            assert self.h, "reference refused the settings"
            self.h = C.c_void_p(self.h)
        else:
            lib = self.lib = lamehip.load_library()
            self.h = C.c_void_p(lib.lame_init())
            lib.lame_set_in_samplerate(self.h, hz)
            lib.lame_set_out_samplerate(self.h, out)
            lib.lame_set_num_channels(self.h, kw.get("channels", 2))
            lib.lame_set_bWriteVbrTag(self.h, 1)
            if "vbr_q" in kw:
                lib.lame_set_VBR(self.h, 4)
                lib.lame_set_VBR_q(self.h, kw["vbr_q"])
            else:
                lib.lame_set_brate(self.h, kw["brate"])
            if "mode" in kw:
                lib.lame_set_mode(self.h, kw["mode"])
            if gain:
                lib.lame_set_findReplayGain(self.h, 1)
            assert lib.lame_init_params(self.h) == 0, lamehip.last_error()
            lib.lame_encode_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            lib.lame_encode_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            lib.lame_get_lametag_frame.restype = C.c_size_t
            lib.lame_get_lametag_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            lib.lame_get_RadioGain.argtypes = [C.c_void_p]

    def call(self, x):
        l, r = np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1])
        if self.ref:
            k = self.ref.lib.refh_encode(self.h, l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), x.shape[1], self.buf,
                                         len(self.buf))
        else:
            k = self.lib.lame_encode_buffer(self.h, l.ctypes.data, r.ctypes.data, x.shape[1], self.buf, len(self.buf))
        assert k >= 0
        return self.buf.raw[:k]

    def flush(self):
        k = self.ref.lib.refh_flush(self.h, self.buf, len(self.buf)) if self.ref else self.lib.lame_encode_flush(self.h, self.buf, len(self.buf))
        assert k >= 0
        return self.buf.raw[:k]

    def tag(self):
        tbuf = C.create_string_buffer(2880)
        k = self.ref.lib.refh_lametag(self.h, tbuf, len(tbuf)) if self.ref else self.lib.lame_get_lametag_frame(self.h, tbuf, len(tbuf))
        return tbuf.raw[:k]

    def radio_gain(self):
        return self.lib.lame_get_RadioGain(self.h)

    def close(self):
        if self.ref:
            self.ref.lib.refh_close(self.h)
        else:
            self.lib.lame_close(self.h)


def yardstick(hz, kw, x, calls, out=OUT, gain=False):
    """stream x through a Handle in `calls': (the audio bytes after every call, cumulative and without the placeholder frame;
    all of them with the flush; the tag frame; the radio gain or None)"""
    h = Handle(hz, kw, out, gain)
    got, upto, at = b"", [], 0
    for n in calls:
        got += h.call(x[:, at:at + n])
        at += n
        upto.append(len(got))
    assert at == x.shape[1]
    got += h.flush()
    tag = h.tag()
    g = h.radio_gain() if gain else None
    h.close()
    assert 0 < len(tag) < len(got)
    return [max(0, u - len(tag)) for u in upto], got[len(tag):], tag, g


def calls_of(n, s):
    """the calls stream s of n samples is fed in: the ragged chunks first, rotated by the stream's number, then 9000 at a time"""
    calls, left, r = [], n, 0
    while left > 0 or r < len(msup.CHUNKS):
        m = min(msup.CHUNKS[(r + s) % len(msup.CHUNKS)] if r < len(msup.CHUNKS) else 9000, left)
        calls.append(m)
        left -= m
        r += 1
    return calls


@functools.lru_cache(maxsize=None)
def pool_data(gain):
    """the pool of nine streams, computed once and left alone: per stream the samples (0.3 .. 0.54 s at its rate), its calls,
    the yardstick's bytes, tag and gain, and the host chain's floats with the converted count after every call"""
    rlib, plib = msup.library(), psup.library()
    enc = t.open_product(OWN, JS128, OUT)
    cfg = enc.config()
    enc.close()
    m = psup.matrix(plib, PCM_S16, cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r)
    streams = []
    for s, hz in enumerate(RATES):
        x = helpers.synth_stream(8100 + s, int(hz * (0.3 + 0.03 * s)), hz, 1.0 / 7)
        calls = calls_of(x.shape[1], s)
        upto, audio, tag, g = yardstick(hz, JS128, x, calls, gain=gain)
        chain, conv, at = msup.chain(rlib, hz, cfg.channels), [], 0
        for n in calls:
            chain.call(psup.host_ingest(plib, PCM_S16, m, x[0, at:at + n], x[1, at:at + n]))
            conv.append(chain.fed)
            at += n
        chain.flush()
        streams.append((x, calls, upto, audio, tag, g, chain.floats(), conv, chain.frames))
    return streams


def open_pool(enc, stype, nstreams, cap, packing=False, gain=False):
    b = lamehip.Batch(enc, nstreams, cap)
    b.set_device_resampling()
    if stype != PCM_S16:
        b.set_sample_type(stype)
    if packing:
        b.set_device_packing()
        b.set_incremental_packing()
    b.set_incremental_resampling()
    if gain:
        b.set_incremental_replaygain()
    if packing:
        b.set_incremental_tagging()
    return b


def run_pool(packing, gain, floats):
    streams = pool_data(gain)
    B = len(streams)
    enc = t.open_product(OWN, JS128, OUT)
    cap = max(x.shape[1] for x, *_ in streams) + 5
    b = open_pool(enc, PCM_S16, B, cap, packing, gain)
    for s, hz in enumerate(RATES):
        b.set_stream_in_samplerate(s, hz)
        assert b.stream_in_samplerate(s) == hz
    got, pos, ms = [b""] * B, [0] * B, 0.0
    for rnd in range(max(len(st[1]) for st in streams)):
        for s, (x, calls, *_) in enumerate(streams):
            n = calls[rnd] if rnd < len(calls) else 0
            b.append(s, x[0, pos[s]:pos[s] + n], x[1, pos[s]:pos[s] + n])
            pos[s] += n
        b.encode_available()
        ms += b.resample_ms()
        taid.drain_all(b, got)
        for s, (x, calls, upto, audio, tag, g, want, conv, frames) in enumerate(streams):
            k = min(rnd, len(calls) - 1)
            assert got[s] == audio[:upto[k]], "round %d stream %d (%d Hz)" % (rnd, s, RATES[s])
            if floats:
                f = b.converted(s)
                assert f.shape[1] == conv[k] and psup.same_floats(f, want[:, :conv[k]]), "round %d stream %d (%d Hz)" % (rnd, s, RATES[s])
    b.finish()
    ms += b.resample_ms()
    taid.drain_all(b, got)
    for s, (x, calls, upto, audio, tag, g, want, conv, frames) in enumerate(streams):
        assert got[s] == audio and len(audio) > 3000, "stream %d (%d Hz)" % (s, RATES[s])
        assert b.frames(s) == frames
        assert psup.same_floats(b.converted(s), want), "stream %d (%d Hz)" % (s, RATES[s])
        if gain:
            assert b.radio_gain(s) == g, "stream %d (%d Hz)" % (s, RATES[s])
        if packing:
            assert b.tag_size() == len(tag) and b.tag(s) == tag, "tag of stream %d (%d Hz)" % (s, RATES[s])
    assert ms > 0.0
    b.close()
    enc.close()


@pytest.mark.parametrize("packing", [False, True], ids=["host-packer", "device-packer-tags"])
def test_pool_of_nine_rates_matches_the_handle_call_by_call(packing):
    """nine streams at 48, 32, 22.05, 88.2, 96, 8, 44.13, 44.1 and 44.11 kHz into one 44.1 kHz joint-stereo CBR 128 batch, fed
    round by round in chunks of 0, 1, 1151, 1152, 1153 and 4000 samples (then 9000 at a time): after every round every
    stream's drains so far are what its handle returned for the same calls, and converted(s) is the host chain at its rate,
    float for float; after finish the flush, the frame counts and -- on the device packer with tagging -- the tag frames"""
    run_pool(packing, False, floats=not packing)


def test_pool_radio_gains_are_the_handles():
    """the same pool with ReplayGain carried round by round, on the device packer with tag frames: radio_gain(s) is
    lame_get_RadioGain of the handle at the stream's rate, and the tag frames carry it"""
    run_pool(True, True, floats=False)


# (id, settings, output rate, the batch's own input rate, the streams' rates)
OTHERS = [
    ("vbr2", dict(vbr_q=2), 44100, 48000, [48000, 32000, 44100, 8000]),
    ("mono", dict(brate=96, channels=1), 44100, 48000, [22050, 48000, 44110, 96000]),
    ("mpeg2-22k", dict(brate=64), 22050, 48000, [48000, 8000, 22050]),
]


@pytest.mark.parametrize("case", range(len(OTHERS)), ids=[c[0] for c in OTHERS])
def test_other_settings(case):
    """-V2, mono, and an MPEG-2 output rate (48 and 8 kHz in, 22.05 kHz out, and a stream already at it): the drains after
    every round are what lame_encode_buffer returned at (in = the stream's rate, out explicit)"""
    _, kw, out, own, rates = OTHERS[case]
    B = len(rates)
    xs = [helpers.synth_stream(8300 + 10 * case + s, int(hz * 0.35) + 17 * s, hz, 1.0 / 7) for s, hz in enumerate(rates)]
    eps = [tard.EntryPoint(PCM_S16, False, hz, kw, out) for hz in rates]
    enc = t.open_product(own, kw, out)
    b = open_pool(enc, PCM_S16, B, max(x.shape[1] for x in xs))
    for s, hz in enumerate(rates):
        b.set_stream_in_samplerate(s, hz)
    calls = [calls_of(x.shape[1], s) for s, x in enumerate(xs)]
    pos = [0] * B
    for rnd in range(max(len(c) for c in calls)):
        want = []
        for s in range(B):
            n = calls[s][rnd] if rnd < len(calls[s]) else 0
            x = xs[s][:, pos[s]:pos[s] + n]
            if enc.channels == 1:
                x = np.stack([x[0], x[0]])
            b.append(s, x[0], x[1])
            want.append(eps[s].call(x))
            pos[s] += n
        b.encode_available()
        for s in range(B):
            assert b.drain(s) == want[s], "round %d stream %d (%d Hz)" % (rnd, s, rates[s])
    b.finish()
    for s in range(B):
        flush = eps[s].flush()
        assert b.drain(s) == flush and len(flush) > 0, "flush of stream %d (%d Hz)" % (s, rates[s])
    b.close()
    enc.close()


def test_float32_from_a_torch_tensor():
    """float32 at +-1.0 from a torch tensor through append_device, in a process of its own where torch takes the device
    first (tests/mixed_rates_child.py): four streams at four rates, ragged rounds, the bytes of
    lame_encode_buffer_ieee_float at each stream's rate"""
    script = os.path.join(helpers.ROOT, "tests", "mixed_rates_child.py")
    r = subprocess.run([sys.executable, script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("mixed rates ok") == 1, r.stdout[-3000:]


def test_slots_change_their_rate():
    """a pool at 22.05 kHz: the stream of slot 0 arrives at 48 kHz, ends alone and is drained -- bytes and tag the handle's at
    48 kHz --; its slot restarts at the batch's own rate, the getter says so, and the next tenant, fed without the setter, is
    the handle's at 22.05 kHz; the one after states 8 kHz.  The neighbours, at 32 kHz and at the batch's rate, go on through
    all of it: their bytes and tags are their handles'."""
    own, cap = 22050, 20000
    enc = t.open_product(own, JS128, OUT)
    b = open_pool(enc, PCM_S16, 3, cap, packing=True)
    tenants = [(48000, 14400), (own, 6000), (8000, 3000)]
    neighbours = {1: 32000, 2: own}
    nx = {s: helpers.synth_stream(8400 + s, 3 * 4000, hz, 1.0 / 7) for s, hz in neighbours.items()}
    nwant = {s: yardstick(hz, JS128, nx[s], [2000] * 6) for s, hz in neighbours.items()}
    b.set_stream_in_samplerate(1, neighbours[1])
    got, npos = [b""] * 3, 0
    for k, (hz, n) in enumerate(tenants):
        x = helpers.synth_stream(8410 + k, n, hz, 1.0 / 7)
        calls = [n // 3, n - n // 3]
        _, audio, tag, _ = yardstick(hz, JS128, x, calls)
        if k == 0:
            b.set_stream_in_samplerate(0, hz)
        elif k == 2:
            assert b.stream_in_samplerate(0) == own
            b.set_stream_in_samplerate(0, hz)
        assert b.stream_in_samplerate(0) == hz
        got[0], at = b"", 0
        for m in calls:
            b.append(0, x[0, at:at + m], x[1, at:at + m])
            at += m
            for s in neighbours:
                b.append(s, nx[s][0, npos:npos + 2000], nx[s][1, npos:npos + 2000])
            npos += 2000
            if at == n:
                b.end_stream(0)
            b.encode_available()
            taid.drain_all(b, got)
        assert b.stream_ended(0)
        assert got[0] == audio and len(audio) > 1000, "tenant %d (%d Hz)" % (k, hz)
        assert b.tag(0) == tag, "tag of tenant %d (%d Hz)" % (k, hz)
        if k < 2:
            b.restart_stream(0)
            assert b.stream_in_samplerate(0) == own
    b.finish()
    taid.drain_all(b, got)
    for s in neighbours:
        assert got[s] == nwant[s][1] and b.tag(s) == nwant[s][2], "neighbour %d" % s
        assert b.stream_in_samplerate(s) == neighbours[s]
    b.reset()
    assert [b.stream_in_samplerate(s) for s in range(3)] == [own] * 3
    b.close()
    enc.close()


def test_the_batchs_own_rate_through_the_setter_changes_nothing():
    """all nine streams at the batch's own rate through the setter: the bytes, round by round, and the floats of a batch that
    never made the call"""
    B = 9
    xs = [helpers.synth_stream(8500 + s, int(OWN * 0.3) + 41 * s, OWN, 1.0 / 7) for s in range(B)]
    enc = t.open_product(OWN, JS128, OUT)
    runs = []
    for stated in (False, True):
        b = open_pool(enc, PCM_S16, B, max(x.shape[1] for x in xs))
        if stated:
            for s in range(B):
                b.set_stream_in_samplerate(s, OWN)
        drains, pos = [], [0] * B
        calls = [calls_of(x.shape[1], s) for s, x in enumerate(xs)]
        for rnd in range(max(len(c) for c in calls)):
            for s in range(B):
                n = calls[s][rnd] if rnd < len(calls[s]) else 0
                b.append(s, xs[s][0, pos[s]:pos[s] + n], xs[s][1, pos[s]:pos[s] + n])
                pos[s] += n
            b.encode_available()
            drains.append([b.drain(s) for s in range(B)])
        b.finish()
        drains.append([b.drain(s) for s in range(B)])
        runs.append((drains, [b.converted(s).tobytes() for s in range(B)]))
        assert [b.stream_in_samplerate(s) for s in range(B)] == [OWN] * B
        b.close()
    enc.close()
    assert runs[0] == runs[1] and all(len(d) > 0 for d in runs[0][0][-1])


def test_refusals_and_the_seventeenth_class():
    """every refusal names the call and leaves the batch usable: a batch without round-by-round conversion, no such stream, a
    rate of 0, a stream that has samples, a finished batch; the whole-stream calls once a stream has a rate of its own; the
    class table holds sixteen rates, the batch's own among them, and refuses one more.  The batch then still encodes."""
    lib = lamehip.load_library()
    fn = lib.lamehip_batch_set_stream_in_samplerate
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int]
    name = b"lamehip_batch_set_stream_in_samplerate"
    x = helpers.synth_stream(8600, 6000, 32000, 1.0 / 7)
    enc = t.open_product(OWN, JS128, OUT)
    # without round-by-round conversion
    b = lamehip.Batch(enc, 2, 6000)
    b.set_device_resampling()
    assert fn(b.b, 0, 32000) == -1 and name in lib.lamehip_last_error() and b"lamehip_batch_set_incremental_resampling" in lib.lamehip_last_error()
    b.close()
    b = open_pool(enc, PCM_S16, 2, 8000)        # (room in the float pool's rows for 6000 samples at 32 kHz, flushed)
    for s, hz in ((2, 32000), (-1, 32000), (0, 0), (0, -8000)):
        assert fn(b.b, s, hz) == -1 and name in lib.lamehip_last_error(), (s, hz)
    assert b.stream_in_samplerate(0) == OWN
    # the whole-stream calls, once a stream has a rate of its own
    b.set_stream_in_samplerate(1, 32000)
    lib.lamehip_batch_set_length.argtypes = [C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_batch_set_pcm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    lib.lamehip_batch_set_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_batch_set_pcm_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    lib.lamehip_batch_set_input_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_batch_encode.argtypes = [C.c_void_p]
    pl, pr, dev = x[0].ctypes.data, x[1].ctypes.data, b.pcm_device_ptr()
    for who, rc in (("lamehip_batch_set_length", lambda: lib.lamehip_batch_set_length(b.b, 0, 100)),
                    ("lamehip_batch_set_pcm", lambda: lib.lamehip_batch_set_pcm(b.b, 0, pl, pr, 100)),
                    ("lamehip_batch_set_input", lambda: lib.lamehip_batch_set_input(b.b, 0, pl, pr, 1, 100)),
                    ("lamehip_batch_set_pcm_device", lambda: lib.lamehip_batch_set_pcm_device(b.b, 0, dev, dev, 100)),
                    ("lamehip_batch_set_input_device", lambda: lib.lamehip_batch_set_input_device(b.b, 0, dev, dev, 1, 100)),
                    ("lamehip_batch_encode", lambda: lib.lamehip_batch_encode(b.b))):
        assert rc() == -1 and who.encode() + b":" in lib.lamehip_last_error() and name in lib.lamehip_last_error(), who
    # a stream that has samples; the other stream still takes a rate
    b.append(1, x[0, :3000], x[1, :3000])
    assert fn(b.b, 1, 22050) == -1 and name in lib.lamehip_last_error() and b"samples" in lib.lamehip_last_error()
    assert b.stream_in_samplerate(1) == 32000
    # sixteen classes: the batch's own, 32 kHz, and fourteen more -- two of them rates that are not converted
    more = [8000, 11025, 12000, 16000, 22050, 24000, 44100, 44110, 64000, 88200, 96000, 37800, 47999, 50000]
    for hz in more:
        b.set_stream_in_samplerate(0, hz)
        assert b.stream_in_samplerate(0) == hz
    assert fn(b.b, 0, 50001) == -1 and name in lib.lamehip_last_error() and b"distinct input rates" in lib.lamehip_last_error()
    assert b.stream_in_samplerate(0) == 50000
    b.set_stream_in_samplerate(0, 8000)                 # (a class that exists is no new one)
    # ... and the batch still works: stream 1 at 32 kHz, stream 0 at 8 kHz
    b.append(1, x[0, 3000:], x[1, 3000:])
    b.append(0, x[0, :1000], x[1, :1000])
    b.encode_available()
    got = [b.drain(0), b.drain(1)]
    b.finish()
    assert fn(b.b, 0, 32000) == -1 and name in lib.lamehip_last_error() and b"finished" in lib.lamehip_last_error()
    got = [got[s] + b.drain(s) for s in range(2)]
    for s, (hz, calls, n) in enumerate(((8000, [1000], 1000), (32000, [3000, 3000], 6000))):
        ep = tard.EntryPoint(PCM_S16, False, hz, JS128, OUT)
        want, at = b"", 0
        for m in calls:
            want += ep.call(x[:, at:at + m])
            at += m
        assert got[s] == want + ep.flush(), "stream %d" % s
    b.close()
    enc.close()
