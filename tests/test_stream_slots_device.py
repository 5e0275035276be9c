"""The slots of an incremental batch (lamehip_batch_end_stream / _stream_ended / _restart_stream, csrc/lh_slots.hip) on the
GPU: utterances that come and go over a few slots, each one's bytes, tag frame and gain against code paths that know nothing
of the slot calls -- a one-shot batch of the utterance's samples, or a fresh one-stream incremental batch ended by finish()
where the bytes depend on how the stream is cut into calls (tests/stream_slots_support.py).  Neighbours that run through the
whole schedule untouched; windows and the fused kernel; edge rounds; finish and reset with ended slots; what is refused.
Every check is byte equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import lamehip
import pcm_input_support as psup
import stream_slots_support as ss
import test_pcm_input_device as t
from lamehip import PCM_F32_UNIT, PCM_S16
from test_incremental_packing_device import CASES

pytestmark = pytest.mark.gpu

SLOTS, UTTERANCES = 6, 14


def make_batch(enc, stype, B, cap, device, tagging=True, gain=False):
    b = lamehip.Batch(enc, B, cap)
    if stype != PCM_S16:
        b.set_sample_type(stype)
    if device:
        b.set_device_packing()
        b.set_incremental_packing()
        if tagging:
            b.set_incremental_tagging()
    if gain:
        b.set_incremental_replaygain()
    return b


def utterances(stype, sr, seed, n=UTTERANCES):
    """n utterances of 0.3 .. 0.9 s, odd lengths"""
    rng = np.random.default_rng(seed)
    lens = [int(sr * rng.uniform(0.3, 0.9)) | 1 for _ in range(n)]
    return lens, [psup.typed_signal(stype, seed + 10 + u, lens[u], sr) for u in range(n)]


def poison_pool(b):
    pool, size = b.bytes_device_ptr()
    assert pool and size > 0
    b.lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert b.lib.hipMemset(pool, 0xA5, size) == 0
    assert b.lib.hipDeviceSynchronize() == 0


# ---- 1. slots that turn over ----

@pytest.mark.parametrize("packer", ["host", "device"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_slots_turn_over(case, packer):
    """14 utterances over 6 slots in ragged chunks (also of 0 and 1 samples); a slot takes the next utterance in the gap behind
    its ending round.  Every utterance's drains are its one-shot bytes; on the device packer with tag frames the tag handed out
    right behind the ending round is the one-shot image's head and completes the image; stream_ended() is 0 before the ending
    round and 1 behind it; tag(s) of a stream that has not ended raises with the message it always had."""
    name, stype, sr, kw = CASES[case]
    device = packer == "device"
    lens, xs = utterances(stype, sr, 6100 + 20 * case)
    rounds = ss.schedule(np.random.default_rng(6200 + case), lens, SLOTS)
    enc = t.open_product(sr, kw)
    mono = enc.channels == 1
    cap = max(lens) + case % 4
    audio, images = ss.one_shot(enc, stype, mono, xs, cap)
    b = make_batch(enc, stype, SLOTS, cap, device)
    T = b.tag_size()
    assert (T > 0) == (device and case != 5)
    res = ss.run_schedule(b, stype, mono, xs, rounds, device)
    ss.check_turnover(res, T, audio, images, device, "%s, %s packer" % (name, packer))
    assert len(res.ending_rounds) >= 3 and any(len(r[1]) == 0 for r in rounds)
    b.close()
    enc.close()


# ---- 2. neighbours are untouched ----

def test_neighbours_are_untouched():
    """Two long streams in slots 6 and 7 run through the whole schedule beside the six turning slots: round by round their
    drains are those of a control batch in which nothing ends; a neighbour's LhStreamState is the same before and after a
    gap in which other slots restarted, and a restarted slot's is that of a freshly created batch's stream."""
    sr, kw, stype = 44100, dict(brate=128), PCM_S16
    lens, xs = utterances(stype, sr, 6500)
    rounds = ss.schedule(np.random.default_rng(6501), lens, SLOTS)
    step = 1152 + 77
    long_len = step * len(rounds)
    longs = {6: helpers.synth_stream(6510, long_len, sr, 1.0 / 5), 7: helpers.synth_stream(6511, long_len, sr, 1.0 / 6)}
    enc = t.open_product(sr, kw)
    cap = max(max(lens), long_len)
    audio, images = ss.one_shot(enc, stype, False, xs, cap)
    b = make_batch(enc, stype, SLOTS + 2, cap, True)
    control = make_batch(enc, stype, 2, cap, True)
    fresh = lamehip.Batch(enc, 1, 1000)
    pristine = ss.get_state(fresh, 0)
    fresh.close()
    gaps = []

    def before_round(r):
        for k, (s, x) in enumerate(sorted(longs.items())):
            b.append(s, x[0, r * step:(r + 1) * step], x[1, r * step:(r + 1) * step])
            control.append(k, x[0, r * step:(r + 1) * step], x[1, r * step:(r + 1) * step])
        control.encode_available()

    def after_round(r):
        for k, s in enumerate(sorted(longs)):
            assert b.drain(s) == control.drain(k), "round %d, neighbour %d" % (r, s)

    def in_gap(r, restarts):
        if not restarts:
            return
        before = [ss.get_state(b, s) for s in sorted(longs)]
        for s, u, nxt in restarts:
            assert ss.get_state(b, s) != pristine
            b.restart_stream(s)
        assert [ss.get_state(b, s) for s in sorted(longs)] == before, "round %d: a neighbour's state moved" % r
        for s, u, nxt in restarts:
            assert ss.get_state(b, s) == pristine, "round %d: slot %d is not a fresh stream's" % (r, s)
        del restarts[:]         # (done here)
        gaps.append(r)

    rounds = [(a, e, list(rs)) for a, e, rs in rounds]
    res = ss.run_schedule(b, stype, False, xs, rounds, True, before_round, after_round, in_gap)
    ss.check_turnover(res, b.tag_size(), audio, images, True, "beside neighbours")
    assert len(gaps) >= 3
    assert b.finish() > 0 and control.finish() > 0
    for k, s in enumerate(sorted(longs)):
        assert b.drain(s) == control.drain(k) and b.tag(s) == control.tag(k)
    b.close()
    control.close()
    enc.close()


# ---- 3. everything on top ----

def test_everything_on_top_fed_from_a_tensor():
    """float32 at +/- 1.0 through append_device from a tensor on the same GPU, 48 -> 44.1 kHz, ReplayGain, device packing and
    tag frames, all round by round, in a process of its own where torch takes the device first (tests/stream_slots_child.py)"""
    child = os.path.join(helpers.ROOT, "tests", "stream_slots_child.py")
    r = subprocess.run([sys.executable, child], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("stream slots ok") == 1, r.stdout[-3000:]


# ---- 4. windows and the fused kernel ----

def test_ending_rounds_in_windows_and_on_the_fused_kernel(monkeypatch):
    """test 1's schedule at one setting, the rounds in windows of one frame, on the split pipeline whole and on the fused kernel
    in turn: ending rounds of each kind, the same bytes and tags"""
    name, stype, sr, kw = CASES[0]
    lens, xs = utterances(stype, sr, 6700)
    rounds = ss.schedule(np.random.default_rng(6701), lens, SLOTS)
    enc = t.open_product(sr, kw)
    cap = max(lens)
    audio, images = ss.one_shot(enc, stype, False, xs, cap)
    b = make_batch(enc, stype, SLOTS, cap, True)
    kinds = {}

    def before_round(r):
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", "1" if r % 3 == 1 else "0")
        monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "1" if r % 3 == 2 else "0")

    def after_round(r):
        kinds[r] = (b.windows(), bool(b.kernel_parts_ms()[0]))

    res = ss.run_schedule(b, stype, False, xs, rounds, True, before_round, after_round)
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "0")
    monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "0")
    ss.check_turnover(res, b.tag_size(), audio, images, True, "windows / fused")
    ending = [kinds[r] for r in res.ending_rounds]
    assert any(w > 1 for w, split in ending) and any(not split for w, split in ending) and any(w == 1 and split for w, split in ending), ending
    b.close()
    enc.close()


# ---- 5. edge rounds ----

def s16_streams(sr, seed, lens):
    return [helpers.synth_stream(seed + u, n, sr, 1.0 / 5) if n else np.zeros((2, 0), np.int16) for u, n in enumerate(lens)]


def test_edge_rounds():
    sr, kw, stype = 44100, dict(vbr_q=4), PCM_S16
    lens = [1000, 15000, 16001, 14003, 20000, 9001]
    xs = s16_streams(sr, 6800, lens)
    enc = t.open_product(sr, kw)
    cap = 40000
    audio, images = ss.one_shot(enc, stype, False, xs, cap)
    b = make_batch(enc, stype, 4, cap, True)
    T = b.tag_size()
    # a round whose only frames are one stream's flush
    b.append(0, xs[0][0], xs[0][1])
    b.end_stream(0)
    with pytest.raises(RuntimeError, match="lamehip_batch_get_tags_all: .*lamehip_batch_finish"):
        b.tags_all()
    assert b.encode_available() == b.frames(0) > 0
    assert b.drain(0) == audio[0] and b.tag(0) == images[0][:T]
    out, sizes = b.tags_all()           # (a negative size for the streams that have not ended)
    assert list(sizes) == [T, -1, -1, -1] and bytes(out[0, :T]) == images[0][:T]
    # a slot that was never fed ends: what a fresh incremental batch finished with nothing appended gives
    b.end_stream(1)
    assert b.encode_available() == b.frames(1) > 0
    nothing = make_batch(enc, stype, 1, cap, True)
    nothing.finish()
    empty = nothing.drain(0)
    assert b.drain(1) == empty and len(empty) > 0 and b.tag(1) == nothing.tag(0) and b.frames(1) == nothing.frames(0)
    nothing.close()
    assert b.restart_ms() == 0.0
    # three slots ended in one round and restarted in one gap: one launch, timed; a round without restarts: 0 again
    b.restart_stream(0)
    b.restart_stream(1)
    for s, u in ((0, 1), (1, 2), (2, 3)):
        b.append(s, xs[u][0], xs[u][1])
        b.end_stream(s)
    b.append(3, xs[4][0, :8000], xs[4][1, :8000])
    b.encode_available()
    assert b.restart_ms() > 0.0         # (slots 0 and 1, restarted in the gap before this round)
    for s, u in ((0, 1), (1, 2), (2, 3)):
        assert b.drain(s) == audio[u] and b.tag(s) == images[u][:T], u
        b.restart_stream(s)
    got4 = b.drain(3)
    b.append(3, xs[4][0, 8000:14000], xs[4][1, 8000:14000])
    b.encode_available()
    assert b.restart_ms() > 0.0
    got4 += b.drain(3)
    b.append(3, xs[4][0, 14000:], xs[4][1, 14000:])
    # an ended stream drained only two rounds after its end: gathered again each round
    b.append(0, xs[5][0], xs[5][1])
    b.end_stream(0)
    b.encode_available()
    assert b.restart_ms() == 0.0
    got4 += b.drain(3)
    assert b.stream_ended(0)
    with pytest.raises(RuntimeError, match="lamehip_batch_restart_stream: .*lamehip_batch_drain"):
        b.restart_stream(0)
    b.append(1, xs[1][0, :7000], xs[1][1, :7000])
    b.encode_available()
    b.append(1, xs[1][0, 7000:], xs[1][1, 7000:])
    b.end_stream(1)
    b.end_stream(3)
    b.encode_available()
    assert bytes(b.drain_view(0)) == audio[5] and b.tag(0) == images[5][:T]
    got4 += b.drain(3)
    assert got4 == audio[4] and b.tag(3) == images[4][:T]
    assert b.drain(1) == audio[1] and b.tag(1) == images[1][:T]
    # every slot has ended and is drained: the byte pool poisoned, the slots' next utterances come out the same
    poison_pool(b)
    for s in (0, 1, 3):
        b.restart_stream(s)
    for s, u in ((0, 2), (1, 3), (3, 0)):
        b.append(s, xs[u][0, :5000], xs[u][1, :5000])
    b.encode_available()
    got = {u: b.drain(s) for s, u in ((0, 2), (1, 3), (3, 0))}
    for s, u in ((0, 2), (1, 3), (3, 0)):
        b.append(s, xs[u][0, 5000:], xs[u][1, 5000:])
        b.end_stream(s)
    b.encode_available()
    for s, u in ((0, 2), (1, 3), (3, 0)):
        assert got[u] + b.drain(s) == audio[u] and b.tag(s) == images[u][:T], u
    b.close()
    enc.close()


# ---- 6. finish and reset with ended slots ----

def solo(enc, stype, cap, chunks, gain):
    """a fresh one-stream incremental batch with the same switches fed the same appends and ended by finish():
    (bytes, tag, radio gain, gain windows)"""
    b = make_batch(enc, stype, 1, cap, True, gain=gain)
    out = b""
    for x in chunks:
        b.append(0, x[0], x[1])
        b.encode_available()
        out += b.drain(0)
    b.finish()
    out += b.drain(0)
    res = (out, b.tag(0), b.radio_gain(0) if gain else None, b.gain_windows(0).tobytes() if gain else None)
    b.close()
    return res


def test_finish_and_reset_with_ended_slots():
    """Streams 0 and 1 end on their own, slot 1 takes another stream; then finish: the rest are flushed, the ended stream's
    tag and gain stay what they were, a second finish is refused; reset, and a second schedule comes out right.  ReplayGain
    round by round on top: the references are one-stream incremental batches fed the same appends."""
    sr, kw, stype = 44100, dict(brate=128), PCM_S16
    lens = [20001, 15000, 30000, 26000, 18001]
    xs = s16_streams(sr, 6900, lens)
    enc = t.open_product(sr, kw)
    cap = 32000
    cut = lambda x, n: [x[:, a:a + n] for a in range(0, x.shape[1], n)]
    pieces = [cut(xs[0], 7000), cut(xs[1], 7000), cut(xs[2], 7000), cut(xs[3], 7000), cut(xs[4], 7000)]
    want = [solo(enc, stype, cap, p, True) for p in pieces]
    b = make_batch(enc, stype, 4, cap, True, gain=True)
    got = {u: b"" for u in range(5)}
    where = {0: 0, 1: 1, 2: 2, 3: 3}            # slot -> utterance
    for r in range(3):
        for s, u in where.items():
            if r < len(pieces[u]):
                b.append(s, pieces[u][r][0], pieces[u][r][1])
                if r == len(pieces[u]) - 1:
                    b.end_stream(s)
        b.encode_available()
        for s, u in where.items():
            got[u] += b.drain(s)
    assert b.stream_ended(0) and b.stream_ended(1) and not b.stream_ended(2) and not b.stream_ended(3)
    for u in (0, 1):
        assert (got[u], b.tag(u), b.radio_gain(u), b.gain_windows(u).tobytes()) == want[u], u
    with pytest.raises(RuntimeError, match="lamehip_batch_radio_gain: .*lamehip_batch_finish"):
        b.radio_gain(2)
    b.restart_stream(1)
    where[1] = 4
    with pytest.raises(RuntimeError, match="lamehip_batch_radio_gain: .*lamehip_batch_finish"):
        b.radio_gain(1)
    assert len(b.gain_windows(1)) == 0
    for r in range(3, 5):
        for s, u in where.items():
            k = r if u != 4 else r - 3
            if s != 0 and k < len(pieces[u]):
                b.append(s, pieces[u][k][0], pieces[u][k][1])
        if r < 4:
            b.encode_available()
            for s, u in where.items():
                got[u] += b.drain(s)
    assert b.finish() > 0
    for s, u in where.items():
        got[u] += b.drain(s)
    # (utterance 4 was cut differently from its reference: two appends, then the flush)
    want[4] = solo(enc, stype, cap, pieces[4][:2], True) if len(pieces[4]) > 2 else want[4]
    for s, u in where.items():
        assert (got[u], b.tag(s), b.radio_gain(s), b.gain_windows(s).tobytes()) == want[u], u
    assert b.stream_ended(0) and b.drain(0) == b""
    with pytest.raises(RuntimeError, match="lamehip_batch_finish: the batch is finished already"):
        b.finish()
    with pytest.raises(RuntimeError, match="lamehip_batch_restart_stream: the batch is finished"):
        b.restart_stream(0)
    # every stream has ended on its own: finish encodes nothing and closes the batch
    b.reset()
    assert not any(b.stream_ended(s) for s in range(4))
    for s in range(4):
        b.end_stream(s)
    b.encode_available()
    assert all(b.stream_ended(s) for s in range(4))
    assert b.finish() == 0
    with pytest.raises(RuntimeError, match="finished"):
        b.encode_available()
    # reset, and a second schedule
    b.reset()
    lens2, xs2 = utterances(stype, sr, 6950, 7)
    lens2 = [min(n, cap) for n in lens2]
    xs2 = [x[:, :n] for x, n in zip(xs2, lens2)]
    audio, images = ss.one_shot(enc, stype, False, xs2, cap)
    # (bytes alone: this batch's tags carry gains, which depend on how a stream is cut into calls)
    res = ss.run_schedule(b, stype, False, xs2, ss.schedule(np.random.default_rng(6951), lens2, 4), False)
    ss.check_turnover(res, b.tag_size(), audio, images, False, "after reset")
    b.close()
    enc.close()


# ---- 7. refusals and messages ----

def test_refusals_and_their_messages():
    sr = 44100
    enc = t.open_product(sr, dict(brate=128))
    lib = enc.lib
    lib.lamehip_last_error.restype = C.c_char_p
    for fn in (lib.lamehip_batch_end_stream, lib.lamehip_batch_restart_stream, lib.lamehip_batch_stream_ended):
        fn.argtypes = [C.c_void_p, C.c_int]
    x = helpers.synth_stream(6990, 9000, sr, 1.0 / 5)
    audio, images = ss.one_shot(enc, PCM_S16, False, [x, x[:, :4000]], 9000)
    err = lambda: lib.lamehip_last_error().decode()
    for device in (False, True):
        b = make_batch(enc, PCM_S16, 2, 9000, device)
        # bad stream indices
        for s in (-1, 2):
            assert lib.lamehip_batch_end_stream(b.b, s) == -1 and "lamehip_batch_end_stream" in err()
            assert lib.lamehip_batch_restart_stream(b.b, s) == -1 and "lamehip_batch_restart_stream" in err()
            assert lib.lamehip_batch_stream_ended(b.b, s) == -1
        assert lib.lamehip_batch_stream_ended(None, 0) == -1
        # restart before anything ended, before the ending round
        assert lib.lamehip_batch_restart_stream(b.b, 0) == -1 and "lamehip_batch_restart_stream: stream 0 has not ended" in err()
        b.append(0, x[0, :5000], x[1, :5000])
        b.end_stream(0)
        assert lib.lamehip_batch_restart_stream(b.b, 0) == -1 and "has not ended" in err()
        # append to an ending stream, every entry point; end twice
        with pytest.raises(RuntimeError, match="lamehip_batch_append: .*lamehip_batch_restart_stream"):
            b.append(0, x[0, :10], x[1, :10])
        with pytest.raises(RuntimeError, match="lamehip_batch_append_input: .*lamehip_batch_restart_stream"):
            b.append_input(0, x[0, :10], x[1, :10])
        assert lib.lamehip_batch_end_stream(b.b, 0) == -1 and "lamehip_batch_end_stream: stream 0 ends with the next round already" in err()
        b.append(1, x[0, :4000], x[1, :4000])
        b.encode_available()
        # append to an ended stream, end it again, restart it undrained
        with pytest.raises(RuntimeError, match="lamehip_batch_append: stream 0 has ended .*lamehip_batch_restart_stream"):
            b.append(0, x[0, :10], x[1, :10])
        assert lib.lamehip_batch_end_stream(b.b, 0) == -1 and "has ended already" in err()
        assert lib.lamehip_batch_restart_stream(b.b, 0) == -1
        assert "lamehip_batch_restart_stream: stream 0 has" in err() and "lamehip_batch_drain" in err()
        # the batch works on: nothing was counted, nothing lost
        assert len(b.drain(0)) > 0
        b.restart_stream(0)
        b.end_stream(1)
        b.encode_available()
        assert b.drain(1) == audio[1]
        b.close()
        b = make_batch(enc, PCM_S16, 1, 9000, device)
        b.append(0, x[0, :5000], x[1, :5000])
        b.end_stream(0)
        b.encode_available()
        first = b.drain(0)
        b.restart_stream(0)
        b.append(0, x[0], x[1])
        b.end_stream(0)
        b.encode_available()
        assert b.drain(0) == audio[0] and first
        # a finished batch
        b.finish()
        assert lib.lamehip_batch_end_stream(b.b, 0) == -1 and "lamehip_batch_end_stream: the batch is finished" in err()
        assert lib.lamehip_batch_restart_stream(b.b, 0) == -1 and "lamehip_batch_restart_stream: the batch is finished" in err()
        b.close()
    # batches on which incremental use is refused: the same checks, the same reasons
    b = lamehip.Batch(enc, 1, 9000)
    b.set_device_packing()
    assert lib.lamehip_batch_end_stream(b.b, 0) == -1
    assert "lamehip_batch_end_stream: incremental batches take" in err() and "lamehip_batch_set_device_packing" in err()
    assert lib.lamehip_batch_restart_stream(b.b, 0) == -1 and "has not ended" in err()
    b.close()
    b = lamehip.Batch(enc, 1, 9000)
    b.set_replaygain()
    assert lib.lamehip_batch_end_stream(b.b, 0) == -1 and "lamehip_batch_end_stream: this batch measures ReplayGain" in err()
    assert lib.lamehip_batch_restart_stream(b.b, 0) == -1
    b.close()
    b = lamehip.Batch(enc, 1, 9000)
    b.set_sample_type(PCM_F32_UNIT)
    assert lib.lamehip_batch_end_stream(b.b, 0) == -1 and "lamehip_batch_end_stream: " in err() and "s16" in err()
    b.close()
    conv = t.open_product(48000, dict(brate=128), 44100)
    b = lamehip.Batch(conv, 1, 9000)
    assert lib.lamehip_batch_end_stream(b.b, 0) == -1 and "converts the sample rate" in err()
    b.close()
    conv.close()
    enc.close()
