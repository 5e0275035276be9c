"""Incremental batches that convert the sample rate on the device (lamehip_batch_set_incremental_resampling;
csrc/lh_resample_dev.hip: lh_resample_tiles_kernel, csrc/lh_ingest.hip: the as-it-is append): every append is one call of
the reference entry point the batch's sample type is named after, converter included, so what a stream drains after a
round is what that call returned, finish is its flush, and converted(s) is lh_rs_block driven call by call; rounds fed from
tensors on the same GPU, a poisoned input pool, launches in windows, the lifecycle and what is refused."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import append_resample_support as asup
import helpers
import lamehip
import pcm_input_support as psup
import resample_support as rsup
import test_append_input_device as taid
import test_pcm_input_device as t
from lamehip import PCM_F32, PCM_F32_UNIT, PCM_S16, PCM_S32

pytestmark = pytest.mark.gpu

# (id, sample type, input rate, settings, output rate asked for or 0, output rate, interleaved)
CASES = [
    ("48k-44k-cbr128-js-f32unit", PCM_F32_UNIT, 48000, dict(brate=128, mode=1), 44100, 44100, False),
    ("44k-48k-cbr128-s16-append", PCM_S16, 44100, dict(brate=128), 48000, 48000, False),
    ("96k-32k-cbr96-s32", PCM_S32, 96000, dict(brate=96), 32000, 32000, False),
    # the output rate left open: the library picks 32 kHz itself -- at 96 kb/s for two channels, and for one channel at the
    # bitrate that is as much per channel, 48 kb/s (mono at 96 kb/s stays at 44.1 kHz, as in the reference: nothing converts)
    ("44k-open-cbr48-mono-f32", PCM_F32, 44100, dict(brate=48, channels=1), 0, 32000, False),
    ("44k-open-cbr96-f32", PCM_F32, 44100, dict(brate=96), 0, 32000, False),
    ("32k-44k-vbr3-f32unit-interleaved", PCM_F32_UNIT, 32000, dict(vbr_q=3), 44100, 44100, True),
    ("48k-44k-downmix-f32unit", PCM_F32_UNIT, 48000, dict(brate=128, mode=3), 44100, 44100, False),
]
IDS = [c[0] for c in CASES]
CHUNKS = [0, 1, 3, 575, 1152, 1153, 4000, 9000]
B = 6


class EntryPoint(taid.EntryPoint):
    """taid.EntryPoint for a handle that converts the rate (open_product / open_reference with their `out' argument), and
    for planar s16 (lame_encode_buffer), which that class has no kind for"""

    def __init__(self, stype, interleaved, sr, kw, out):
        self.planar_s16 = (stype == PCM_S16 and not interleaved)
        self.kind = None if self.planar_s16 else psup.REF_KIND[(stype, interleaved)]
        self.interleaved = interleaved
        self.buf = C.create_string_buffer(200000)
        if helpers.have_reference():
            self.ref, self.enc = helpers.Reference(), None
            self.h = t.open_reference(self.ref, sr, kw, out)
        else:
            self.ref, self.enc = None, t.open_product(sr, kw, out)
            self.fn = getattr(self.enc.lib, "lame_encode_buffer" if self.planar_s16 else psup.HANDLE_CALL[self.kind])
            self.fn.restype = C.c_int

    def call(self, x):
        if not self.planar_s16:
            return super().call(x)
        n = x.shape[1]
        a, b = np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1])
        pa, pb = C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data)
        if self.ref:
            k = self.ref.lib.refh_encode(self.h, pa, pb, n, self.buf, len(self.buf))
        else:
            k = self.fn(self.enc.h, pa, pb, n, self.buf, len(self.buf))
        assert k >= 0
        return self.buf.raw[:k]


def open_batch(enc, stype, nstreams, cap):
    b = lamehip.Batch(enc, nstreams, cap)
    b.set_device_resampling()
    if stype != PCM_S16:
        b.set_sample_type(stype)
    b.set_incremental_resampling()
    return b


def append_chunk(b, stype, s, x, interleaved, mono):
    if stype == PCM_S16 and not interleaved:
        b.append(s, np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1]))        # lamehip_batch_append
    else:
        taid.append_chunk(b, s, x, interleaved, mono)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """per entry of CASES, computed once and left alone: the streams, the chunk every stream gets in every round, what the
    entry point returned for each of those calls and for the flush, and the host chain's floats (lh_rs_block call by
    call, then the flush, over the samples behind the PCM matrix)"""
    _, stype, sr, kw, out, rate_out, interleaved = CASES[case]
    rng = np.random.default_rng(7800 + case)
    lens = [int(sr * 0.5) + 37 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9800 + 10 * case + s, lens[s], sr) for s in range(B)]
    enc = t.open_product(sr, kw, out)
    cfg = enc.config()
    enc.close()
    assert cfg.samplerate == rate_out
    plib, rlib = psup.library(), asup.library()
    m = psup.matrix(plib, stype, cfg.pcm_scale, cfg.pcm_mix, cfg.pcm_scale_r)
    one_plane = cfg.channels == 1 and cfg.pcm_mix == 0.0
    eps = [EntryPoint(stype, interleaved, sr, kw, out) for _ in range(B)]
    chains = [asup.HostChain(rlib, sr, rate_out, cfg.channels) for _ in range(B)]
    pos, rounds = [0] * B, []
    while any(pos[s] < lens[s] for s in range(B)):
        ns = [min(int(rng.choice(CHUNKS)), lens[s] - pos[s]) for s in range(B)]
        want, conv = [], []
        for s in range(B):
            x = xs[s][:, pos[s]:pos[s] + ns[s]]
            want.append(eps[s].call(x))
            chains[s].call(psup.host_ingest(plib, stype, m, x[0], None if one_plane else x[1]))
            conv.append(chains[s].fed)
            pos[s] += ns[s]
        rounds.append((ns, want, conv))
    flushes = [ep.flush() for ep in eps]
    for c in chains:
        c.flush()
    floats = [c.floats() for c in chains]
    frames = [c.frames for c in chains]
    assert len(rounds) > 3 and sum(len(w) for _, want, _ in rounds for w in want) > B * 2000
    return xs, rounds, flushes, floats, frames


def poison_pool(b, stype, nstreams, cap):
    """the whole input pool, through pcm_device_ptr: NaN (0x7fff) everywhere"""
    lib = lamehip.load_library()
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.full((nstreams, 2, cap), psup.beyond_value(stype), lamehip.PCM_DTYPES[stype])
    assert lib.hipMemcpy(b.pcm_device_ptr(), host.ctypes.data, host.nbytes, 1) == 0     # 1 = hipMemcpyHostToDevice


def run_call_by_call(case, poison):
    _, stype, sr, kw, out, rate_out, interleaved = CASES[case]
    xs, rounds, flushes, floats, frames = case_data(case)
    enc = t.open_product(sr, kw, out)
    cap = max(x.shape[1] for x in xs) + case % 4
    b = open_batch(enc, stype, B, cap)
    if poison:
        poison_pool(b, stype, B, cap)
    pos, ms = [0] * B, 0.0
    for rnd, (ns, want, conv) in enumerate(rounds):
        for s in range(B):
            append_chunk(b, stype, s, xs[s][:, pos[s]:pos[s] + ns[s]], interleaved, enc.channels == 1)
            pos[s] += ns[s]
        b.encode_available()
        ms += b.resample_ms()
        for s in range(B):
            assert b.drain(s) == want[s], "round %d stream %d" % (rnd, s)
            got = b.converted(s)
            assert got.shape[1] == conv[s] and psup.same_floats(got, floats[s][:, :conv[s]]), "round %d stream %d" % (rnd, s)
    b.finish()
    ms += b.resample_ms()
    for s in range(B):
        assert b.drain(s) == flushes[s], "flush of stream %d" % s
        assert psup.same_floats(b.converted(s), floats[s]), "stream %d" % s
        assert b.frames(s) == frames[s]
    assert ms > 0.0
    b.close()
    enc.close()


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_appends_match_the_entry_point_call_by_call(case):
    """six streams of 0.5 s + 37 s input samples fed in ragged chunks (also empty ones), one encode_available per round: what
    every stream drains after a round is what the entry point returned for that stream's call of the round, finish is its
    flush, and converted(s) is the host chain float for float after every round"""
    run_call_by_call(case, poison=False)


@pytest.mark.parametrize("case", [0, 1, 3], ids=[IDS[0], IDS[1], IDS[3]])
def test_poisoned_input_pool_changes_nothing(case):
    """the input pool filled with NaN (0x7fff) through pcm_device_ptr before the first append -- the right rows of the mono
    case stay that way --: nothing at or beyond what a stream has been fed is read, the bytes and floats are unchanged"""
    run_call_by_call(case, poison=True)


def child(mode, env=None):
    script = os.path.join(helpers.ROOT, "tests", "append_resample_child.py")
    r = subprocess.run([sys.executable, script, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("incremental conversion ok") == 1, r.stdout[-3000:]


def test_mixed_sources_from_torch():
    """four float32 streams at 48 -> 44.1 kHz, 1152 samples per append, in a process of its own where torch takes the device
    first (tests/append_resample_child.py): rounds through append_device from a [B, 2, T] tensor, a view of a larger one
    and an interleaved one, and per stream through append_input with tensor slices, the other stream of each pair from
    host arrays -- the bytes of the one-shot whole-stream batch, whose plan is the reference fed 1152 per call"""
    child("mixed")


def test_launches_in_windows():
    """the same with LAMEHIP_MID_WINDOW=3 in the child's environment: the encode launches behind the conversion run in
    windows of frames, same bytes"""
    child("window", {"LAMEHIP_MID_WINDOW": "3"})


def test_reset_and_finish():
    """reset followed by a second run gives the same bytes; an append after finish is refused until then"""
    stype, sr, out = PCM_F32_UNIT, 48000, 44100
    x = psup.typed_signal(stype, 9900, 9000, sr)
    enc = t.open_product(sr, dict(brate=128), out)
    b = open_batch(enc, stype, 2, 9000)
    runs = []
    for attempt in range(2):
        got = [b"", b""]
        for a, e in ((0, 4000), (4000, 4001), (4001, 9000)):
            b.append_input(0, x[0, a:e], x[1, a:e])
            b.append_input(1, interleaved=np.ascontiguousarray(x[:, a:e].T))
            b.encode_available()
            taid.drain_all(b, got)
        b.finish()
        taid.drain_all(b, got)
        assert got[0] == got[1] and len(got[0]) > 2000
        runs.append((got, b.converted(0)))
        with pytest.raises(RuntimeError, match="finished"):
            b.append_input(0, x[0, :10], x[1, :10])
        b.reset()
    assert runs[0][0] == runs[1][0] and psup.same_floats(runs[0][1], runs[1][1])
    b.close()
    enc.close()


def test_refusals():
    """the switch on a batch that does not convert, without device resampling, after PCM was handed over; the appends with
    device packing or ReplayGain on top of it; an append whose flushed stream would exceed the float pool (nothing counted,
    the batch usable, finish succeeds); lamehip_batch_append (shorts) on a typed batch -- -1 and a message every time"""
    lib = lamehip.load_library()
    lib.lamehip_batch_set_incremental_resampling.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.lamehip_batch_append_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.lamehip_batch_append_input_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.lamehip_batch_append_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
    stype, sr, out = PCM_F32_UNIT, 48000, 44100
    x = psup.typed_signal(stype, 9910, 6000, sr)
    shorts = helpers.synth_stream(9911, 6000, sr)
    pl, pr = x[0].ctypes.data, x[1].ctypes.data
    lengths = (C.c_int * 1)(10)
    # a batch that does not convert
    plain = t.open_product(44100, dict(brate=128))
    b = lamehip.Batch(plain, 1, 6000)
    assert lib.lamehip_batch_set_incremental_resampling(b.b, 1) == -1
    assert b"lamehip_batch_set_device_resampling" in lib.lamehip_last_error()
    b.close()
    plain.close()
    enc = t.open_product(sr, dict(brate=128), out)
    # without device resampling; after PCM was handed over
    b = lamehip.Batch(enc, 1, 6000)
    assert lib.lamehip_batch_set_incremental_resampling(b.b, 1) == -1
    assert b"lamehip_batch_set_device_resampling" in lib.lamehip_last_error()
    b.set_device_resampling()
    b.set_pcm(0, shorts[0], shorts[1])
    assert lib.lamehip_batch_set_incremental_resampling(b.b, 1) == -1
    assert b"before any PCM" in lib.lamehip_last_error()
    b.close()
    # device packing or ReplayGain on top of the switch: the appends are refused, the batch still takes whole streams
    for what in ("packing", "replaygain"):
        b = open_batch(enc, stype, 1, 6000)
        if what == "packing":
            b.set_device_packing()
        else:
            b.set_replaygain()
        dev = b.pcm_device_ptr()
        for name, (a0, a1) in (("lamehip_batch_append_input", (pl, pr)), ("lamehip_batch_append_input_device", (dev, dev))):
            assert getattr(lib, name)(b.b, 0, a0, a1, 1, 100) == -1
            assert name.encode() + b":" in lib.lamehip_last_error(), what
        assert lib.lamehip_batch_append_device(b.b, dev, 0, 0, 1, lengths) == -1
        assert b"lamehip_batch_append_device:" in lib.lamehip_last_error(), what
        b.set_input(0, x[0], x[1])
        b.encode()
        assert len(b.pack(0)) > 0, what
        b.close()
    # shorts on a typed batch
    b = open_batch(enc, stype, 1, 6000)
    assert lib.lamehip_batch_append(b.b, 0, shorts[0].ctypes.data, shorts[1].ctypes.data, 100) == -1
    assert b"lamehip_batch_append:" in lib.lamehip_last_error()
    b.close()
    enc.close()


def flushed_length(rlib, rs, calls):
    """converted samples of a stream fed `calls' and then flushed, from the plan"""
    cur = asup.cursor(rlib)
    for m in calls:
        asup.plan_call(rlib, rs, cur, m)
    asup.plan_flush(rlib, rs, cur)
    return cur.fed


def test_append_that_would_not_leave_room_for_the_flush(monkeypatch):
    """An append is refused when its stream, flushed right after the call, would exceed the float pool: -1, the call named,
    nothing counted, the batch usable, and finish afterwards succeeds.  The pool's own margin holds the flush of any stream
    within the input capacity, so the appends are told of a smaller pool (LAMEHIP_INC_RS_ROOM, a test aid): which calls fit
    follows from the plan."""
    lib = lamehip.load_library()
    lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    sr, out, room = 48000, 44100, 6000
    rlib = asup.library()
    rs = rsup.resampler(rlib, sr, out)
    assert flushed_length(rlib, rs, [3000]) <= room < flushed_length(rlib, rs, [3000, 3000])
    assert flushed_length(rlib, rs, [3000, 1]) <= room < flushed_length(rlib, rs, [3000, 1, 2999])
    xs = helpers.synth_stream(9912, 6000, sr)
    enc = t.open_product(sr, dict(brate=128), out)
    monkeypatch.setenv("LAMEHIP_INC_RS_ROOM", str(room))
    b = lamehip.Batch(enc, 2, 6000)
    b.set_device_resampling()
    b.set_incremental_resampling()
    monkeypatch.delenv("LAMEHIP_INC_RS_ROOM")
    got = [b"", b""]
    for s in range(2):
        b.append(s, xs[0, :3000], xs[1, :3000])
    for n in (3000, 2999):
        assert lib.lamehip_batch_append(b.b, 0, xs[0, 3000:].ctypes.data, xs[1, 3000:].ctypes.data, n) == -1
        assert b"lamehip_batch_append:" in lib.lamehip_last_error() and b"float pool" in lib.lamehip_last_error()
        b.append(0, xs[0, 3000:3000], xs[1, 3000:3000])         # (an empty call always fits)
        b.append(1, xs[0, 3000:3000], xs[1, 3000:3000])
    assert lib.lamehip_batch_append(b.b, 0, xs[0].ctypes.data, xs[1].ctypes.data, 3001) == -1      # the input capacity
    assert b"capacity" in lib.lamehip_last_error()
    b.encode_available()
    taid.drain_all(b, got)
    for s in range(2):
        b.append(s, xs[0, 3000:3001], xs[1, 3000:3001])
    assert lib.lamehip_batch_append(b.b, 0, xs[0, 3001:].ctypes.data, xs[1, 3001:].ctypes.data, 2999) == -1
    assert b"float pool" in lib.lamehip_last_error()
    b.finish()
    taid.drain_all(b, got)
    # the refused calls counted nothing: stream 0, which met them, gives what stream 1 gives, which is the entry point's
    ep = EntryPoint(PCM_S16, False, sr, dict(brate=128), out)
    want = ep.call(xs[:, :3000]) + ep.call(xs[:, :0]) + ep.call(xs[:, :0]) + ep.call(xs[:, 3000:3001]) + ep.flush()
    assert got[0] == got[1] == want and len(want) > 1000
    b.close()
    enc.close()
