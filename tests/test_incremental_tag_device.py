"""Tag frames of an incremental batch on the device packer (lamehip_batch_set_incremental_tagging, csrc/lh_tag.hip:
lh_tag_resume_kernel) on the GPU: after finish every stream's tag is the frame a one-shot batch fed the same samples puts in
front of the stream -- made on the device (get_bytes_tagged of a device-packed batch) and on the host (pack_tagged) --, and
tag_size() zeros followed by all drains, with the tag written over the head, is that whole image; streams long enough for the
bag to halve once and twice, rounds in windows and on the fused kernel; a stream drained only at the end; ReplayGain and
conversion round by round on top; a poisoned byte pool; reset; what is refused; the switch taken back.  Every check is byte
equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import lamehip
import pcm_input_support as psup
import test_pcm_input_device as t
from lamehip import PCM_S16
from test_append_input_device import CHUNKS, append_chunk
from test_incremental_packing_device import CASES, ragged_plan

pytestmark = pytest.mark.gpu


def tagging_batch(enc, stype, B, cap, tagging=True):
    b = lamehip.Batch(enc, B, cap)
    if stype != PCM_S16:
        b.set_sample_type(stype)
    b.set_device_packing()
    b.set_incremental_packing()
    if tagging:
        b.set_incremental_tagging()
    return b


def one_shot_images(enc, stype, xs, cap, device, gain=False):
    """the file images of a whole-stream batch of the same samples: device == True: packed and tagged on the device
    (get_bytes_tagged), else packed and tagged on the host (pack_tagged)"""
    b = lamehip.Batch(enc, len(xs), cap)
    if device:
        b.set_device_packing()
        b.set_device_tagging()
    if stype != PCM_S16:
        b.set_sample_type(stype)
    if gain:
        b.set_replaygain()
    t.feed(b, xs, False, enc.channels == 1)
    b.encode()
    out = [b.get_bytes_tagged(s) if device else b.pack_tagged(s) for s in range(len(xs))]
    b.close()
    return out


def check_tags(b, drained, images, what=""):
    """after finish: tag(s), tags_all() and the image put together from the drains, against the one-shot images (a setting
    whose tag does not fit a frame has tag_size() 0 and no tags: the images are the audio alone, as on the one-shot path)"""
    T = b.tag_size()
    out, sizes = b.tags_all()
    for s, img in enumerate(images):
        tag = b.tag(s)
        assert len(tag) == T and sizes[s] == T and bytes(out[s, :T]) == tag, (what, s)
        assert tag == img[:T], "%s: tag of stream %d" % (what, s)
        assert tag != bytes(T) or T == 0
        whole = bytearray(T) + drained[s]
        whole[:T] = tag
        assert bytes(whole) == img, "%s: image of stream %d" % (what, s)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_tags_match_the_one_shot_images(case):
    """eight streams of 0.9 s + 37 s samples in ragged chunks (also empty ones), through the entry point the sample type is
    named after (MPEG-2.5 at 16 kb/s: the tag does not fit a frame, the batch has no tags and launches nothing for them)"""
    _, stype, sr, kw = CASES[case]
    B = 8
    rng = np.random.default_rng(8850 + case)
    lens = [int(sr * 0.9) + 37 * s for s in range(B)]
    xs = [psup.typed_signal(stype, 9700 + 10 * case + s, lens[s], sr) for s in range(B)]
    enc = t.open_product(sr, kw)
    cap = max(lens) + case % 4
    b = tagging_batch(enc, stype, B, cap)
    T = b.tag_size()
    pos, drained, ms = [0] * B, [b""] * B, 0.0
    while any(pos[s] < lens[s] for s in range(B)):
        for s in range(B):
            n = min(int(rng.choice(CHUNKS)), lens[s] - pos[s])
            append_chunk(b, s, xs[s][:, pos[s]:pos[s] + n], False, enc.channels == 1)
            pos[s] += n
        frames = b.encode_available()
        assert (b.tag_ms() > 0.0) == (frames > 0 and T > 0)
        ms += b.tag_ms()
        assert b.tag_size() == T
        with pytest.raises(RuntimeError, match="lamehip_batch_finish"):
            b.tag(0)
        for s in range(B):
            drained[s] += b.drain(s)
    b.finish()
    assert (b.tag_ms() > 0.0 and ms > 0.0) == (T > 0) and (T > 0) == (case != 5)
    for s in range(B):
        drained[s] += b.drain(s)
    on_device = one_shot_images(enc, stype, xs, cap, True)
    on_host = one_shot_images(enc, stype, xs, cap, False)
    assert on_device == on_host
    check_tags(b, drained, on_device, CASES[case][0])
    b.close()
    enc.close()


@pytest.mark.parametrize("name,kw", [("cbr128", dict(brate=128)), ("V4", dict(vbr_q=4))])
def test_the_bag_halves_on_the_device(name, kw, monkeypatch):
    """two streams at 48 kHz, one of about 500 frames (the bag halves once) and one of about 830 (twice), in rounds of about a second
    that go in windows of frames, on the split pipeline and on the fused kernel in turn"""
    sr, B = 48000, 2
    lens = [500 * 1152 - 700, 830 * 1152 - 300]
    xs = [helpers.synth_stream(9400 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    enc = t.open_product(sr, kw)
    cap = max(lens) + 1
    b = tagging_batch(enc, PCM_S16, B, cap)
    pos, rnd, drained, windows, split = 0, 0, [b""] * B, [], []
    while pos < max(lens):
        n = 47000 + 1152 * (rnd % 3)
        for s in range(B):
            a, e = min(pos, lens[s]), min(pos + n, lens[s])
            if e > a:
                b.append(s, xs[s][0, a:e], xs[s][1, a:e])
        monkeypatch.setenv("LAMEHIP_MID_WINDOW", "16" if rnd % 3 == 1 else "0")
        monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "1" if rnd % 3 == 2 else "0")
        b.encode_available()
        windows.append(b.windows())
        split.append(bool(b.kernel_parts_ms()[0]))
        for s in range(B):
            drained[s] += b.drain(s)
        pos += n
        rnd += 1
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "2")
    monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "0")
    b.finish()
    for s in range(B):
        drained[s] += b.drain(s)
    assert 401 <= b.frames(0) <= 799 and 801 <= b.frames(1) < 1600, [b.frames(s) for s in range(B)]
    assert max(windows) > 1 and min(windows) == 1 and True in split and False in split, (windows, split)
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "0")
    check_tags(b, drained, one_shot_images(enc, PCM_S16, xs, cap, True), name)
    b.close()
    enc.close()


def s16_run(b, xs, plan, drain_late=(), piece=None):
    """feeds xs by `plan' (rounds of per-stream counts; piece: in appends of that many samples), drains every stream after
    every round but those of drain_late, finishes, drains all; returns the streams' bytes"""
    B = len(xs)
    pos, out = [0] * B, [b""] * B
    for ns in plan:
        for s in range(B):
            step = piece or max(ns[s], 1)
            for a in range(pos[s], pos[s] + ns[s], step):
                e = min(a + step, pos[s] + ns[s])
                b.append(s, xs[s][0, a:e], xs[s][1, a:e])
            pos[s] += ns[s]
        b.encode_available()
        for s in range(B):
            if s not in drain_late:
                out[s] += b.drain(s)
    b.finish()
    for s in range(B):
        out[s] += b.drain(s)
    return out


def test_a_stream_drained_only_at_the_end_and_a_poisoned_pool():
    """stream 1 is not drained before finish: its bytes are gathered again every round, its tag is the same; and the same
    run over a byte pool filled with 0xA5 behind the first append (which lays the pool out): the same tags"""
    sr, B = 44100, 3
    rng = np.random.default_rng(8860)
    lens = [int(sr * 0.9) + 37 * s for s in range(B)]
    xs = [helpers.synth_stream(9410 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    plan = ragged_plan(rng, lens)
    enc = t.open_product(sr, dict(vbr_q=2))
    images = one_shot_images(enc, PCM_S16, xs, max(lens), True)
    b = tagging_batch(enc, PCM_S16, B, max(lens))
    drained = s16_run(b, xs, plan, drain_late=(1,))
    check_tags(b, drained, images, "late drain")
    b.close()
    b = tagging_batch(enc, PCM_S16, B, max(lens))
    b.append(0, xs[0][0, :0], xs[0][1, :0])
    pool, size = b.bytes_device_ptr()
    assert pool and size >= B * len(images[0]) // 2
    b.lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert b.lib.hipMemset(pool, 0xA5, size) == 0
    assert b.lib.hipDeviceSynchronize() == 0
    drained = s16_run(b, xs, plan)
    assert b.bytes_device_ptr() == (pool, size)
    check_tags(b, drained, images, "poisoned pool")
    b.close()
    enc.close()


def test_replaygain_round_by_round_on_top():
    """lamehip_batch_set_incremental_replaygain on top, the streams fed a frame's worth per append -- the calls a one-shot
    batch's analysis stands for --: the tag carries the gain a one-shot batch with set_replaygain and device tagging puts in
    its image, and differs from the tag without it in the gain field and the frame's CRC only"""
    sr, B = 44100, 4
    lens = [int(sr * (0.9 + 0.3 * s)) for s in range(B)]
    xs = [helpers.synth_stream(9420 + s, lens[s], sr, 1.0 / 4) for s in range(B)]
    enc = t.open_product(sr, dict(brate=128))
    cap = max(lens)
    plan, pos = [], [0] * B
    while any(p < n for p, n in zip(pos, lens)):
        ns = [min(1152 * (3 + (len(plan) + s) % 4), lens[s] - pos[s]) for s in range(B)]
        pos = [p + n for p, n in zip(pos, ns)]
        plan.append(ns)
    with_gain = one_shot_images(enc, PCM_S16, xs, cap, True, gain=True)
    without = one_shot_images(enc, PCM_S16, xs, cap, True)
    b = tagging_batch(enc, PCM_S16, B, cap)
    b.set_incremental_replaygain()
    drained = s16_run(b, xs, plan, piece=1152)
    check_tags(b, drained, with_gain, "replaygain")
    assert [b.tag(s) for s in range(B)] == [img[:b.tag_size()] for img in with_gain]    # (handed out twice: patched once)
    at = enc.config().sideinfo_len + 116
    for s in range(B):
        differ = [i for i in range(b.tag_size()) if with_gain[s][i] != without[s][i]]
        assert differ and set(differ) <= {at + 19, at + 20, at + 38, at + 39}, differ
    b.close()
    enc.close()


def test_conversion_on_top_fed_from_a_tensor():
    """float32 at +/- 1.0 through append_device from a tensor on the same GPU, 48 -> 44.1 kHz round by round on top of the
    switch, in a process of its own where torch takes the device first (tests/incremental_tag_child.py): the tags of the
    one-shot batch that converts on the device"""
    child = os.path.join(helpers.ROOT, "tests", "incremental_tag_child.py")
    r = subprocess.run([sys.executable, child], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.count("incremental tagging ok") == 1, r.stdout[-3000:]


def test_reset_and_a_second_run():
    """finish, reset, other and shorter streams: no tag until the second finish, then the second streams' tags"""
    sr, B = 44100, 3
    enc = t.open_product(sr, dict(brate=160))
    cap = int(sr * 1.1)
    b = tagging_batch(enc, PCM_S16, B, cap)
    for run, secs in enumerate((1.0, 0.6)):
        lens = [int(sr * secs) + 411 * s for s in range(B)]
        xs = [helpers.synth_stream(9430 + 10 * run + s, lens[s], sr, 1.0 / 5) for s in range(B)]
        plan = ragged_plan(np.random.default_rng(8870 + run), lens)
        with pytest.raises(RuntimeError, match="lamehip_batch_finish"):
            b.tag(0)
        with pytest.raises(RuntimeError, match="lamehip_batch_finish"):
            b.tags_all()
        drained = s16_run(b, xs, plan)
        check_tags(b, drained, one_shot_images(enc, PCM_S16, xs, cap, True), "run %d" % run)
        b.reset()
    b.close()
    enc.close()


def test_refusals_and_their_messages():
    sr = 44100
    enc = t.open_product(sr, dict(brate=128))
    lib = enc.lib
    fn = lib.lamehip_batch_set_incremental_tagging
    fn.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_last_error.restype = C.c_char_p
    lib.lamehip_batch_set_incremental_packing.argtypes = [C.c_void_p, C.c_int]
    x = helpers.synth_stream(9440, 6000, sr, 1.0 / 5)
    # without incremental packing: a plain batch, a device-packed one
    b = lamehip.Batch(enc, 1, 6000)
    assert fn(b.b, 1) == -1
    assert b"lamehip_batch_set_incremental_tagging:" in lib.lamehip_last_error() and b"lamehip_batch_set_incremental_packing" in lib.lamehip_last_error()
    b.set_device_packing()
    assert fn(b.b, 1) == -1
    assert b"lamehip_batch_set_incremental_tagging:" in lib.lamehip_last_error() and b"lamehip_batch_set_incremental_packing" in lib.lamehip_last_error()
    assert b.tag_size() == 0
    with pytest.raises(RuntimeError, match="lamehip_batch_tag_ptr: lamehip_batch_set_incremental_tagging is not on"):
        b.tag(0)
    # behind it: accepted; the one-shot switch stays refused, with its message; incremental packing cannot be taken away
    b.set_incremental_packing()
    assert fn(b.b, 1) == 0 and b.tag_size() == 417
    with pytest.raises(RuntimeError, match="an incremental batch has no tagged output"):
        b.set_device_tagging()
    assert lib.lamehip_batch_set_incremental_packing(b.b, 0) == -1
    assert b"lamehip_batch_set_incremental_packing:" in lib.lamehip_last_error() and b"lamehip_batch_set_incremental_tagging" in lib.lamehip_last_error()
    # on = 0 puts the batch back: no tags, and incremental packing can go
    assert fn(b.b, 0) == 0 and b.tag_size() == 0
    assert lib.lamehip_batch_set_incremental_packing(b.b, 0) == 0
    assert fn(b.b, 1) == -1
    b.set_incremental_packing()
    assert fn(b.b, 1) == 0
    # not once the batch is fed
    b.append(0, x[0, :3000], x[1, :3000])
    for on in (0, 1):
        assert fn(b.b, on) == -1
        assert b"lamehip_batch_set_incremental_tagging: only before any PCM" in lib.lamehip_last_error()
    # a round without a complete frame launches nothing; one with frames does
    assert b.encode_available() > 0 and b.tag_ms() > 0.0
    b.append(0, x[0, :0], x[1, :0])
    assert b.encode_available() == 0 and b.tag_ms() == 0.0 and b.drain_ms() == 0.0
    with pytest.raises(RuntimeError, match="lamehip_batch_tag_ptr: .*lamehip_batch_finish"):
        b.tag(0)
    with pytest.raises(RuntimeError, match="lamehip_batch_get_tags_all: .*lamehip_batch_finish"):
        b.tags_all()
    b.finish()
    assert len(b.tag(0)) == 417
    lib.lamehip_batch_tag_ptr.restype = C.c_long
    lib.lamehip_batch_tag_ptr.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    p = C.c_void_p()
    assert lib.lamehip_batch_tag_ptr(b.b, 1, C.byref(p)) == -1 and lib.lamehip_batch_tag_ptr(b.b, 0, None) == -1
    b.close()
    # after PCM was handed over whole
    b = lamehip.Batch(enc, 1, 6000)
    b.set_device_packing()
    b.set_incremental_packing()
    b.set_pcm(0, x[0], x[1])
    assert fn(b.b, 1) == -1
    assert b"before any PCM" in lib.lamehip_last_error()
    b.close()
    enc.close()


def test_the_switch_taken_back_changes_nothing():
    """switched on and off again before the first append, the batch is the one that never saw the switch: the same drains
    round by round, no tag launch (tag_ms() stays 0), no tag size, no tags.  (The library has no launch counter: the tag
    launch is the only one the switch adds, and its events are the evidence that it did not run.)"""
    sr, B = 44100, 4
    rng = np.random.default_rng(8880)
    lens = [int(sr * 0.7) + 37 * s for s in range(B)]
    xs = [helpers.synth_stream(9450 + s, lens[s], sr, 1.0 / 5) for s in range(B)]
    plan = ragged_plan(rng, lens)
    enc = t.open_product(sr, dict(vbr_q=3))
    never = tagging_batch(enc, PCM_S16, B, max(lens), tagging=False)
    back = tagging_batch(enc, PCM_S16, B, max(lens))
    back.set_incremental_tagging(False)
    pos = [0] * B
    for ns in plan + [None]:
        for b in (never, back):
            if ns is None:
                b.finish()
            else:
                for s in range(B):
                    b.append(s, xs[s][0, pos[s]:pos[s] + ns[s]], xs[s][1, pos[s]:pos[s] + ns[s]])
                b.encode_available()
            assert b.tag_ms() == 0.0 and b.tag_size() == 0
        if ns is not None:
            pos = [p + n for p, n in zip(pos, ns)]
        for s in range(B):
            assert back.drain(s) == never.drain(s), s
    with pytest.raises(RuntimeError, match="not on"):
        back.tag(0)
    never.close()
    back.close()
    enc.close()
