"""What tests/test_stream_slots_device.py and tests/stream_slots_child.py share: a schedule of utterances over the slots of
an incremental batch -- made on the host from a seed, before any batch exists --, the loop that carries it out (append, end,
round, drain + tag, restart), and the references the slot path is compared against, all of them paths that do not know the
slot calls: a one-shot batch of the utterances' samples, and a fresh one-stream incremental batch ended by finish()."""
import ctypes as C

import numpy as np
import pytest

import lamehip
from lamehip import PCM_S16

CHUNKS = [0, 1, 3, 575, 1152, 1153, 4000, 9000]


def schedule(rng, lens, B, chunks=CHUNKS):
    """Utterances 0 .. len(lens) - 1 over B slots: every round a live slot gets a chunk from `chunks' (also 0 samples) of
    its utterance; the slot whose utterance is through ends with that round and takes the next utterance in the gap behind
    it.  Returns the rounds: (appends [(slot, utterance, a, e)], ending slots, restarts [(slot, utterance that ended, next
    utterance or None)])."""
    queue = list(range(len(lens)))
    cur = [queue.pop(0) if queue else None for _ in range(B)]
    pos = [0] * B
    rounds = []
    while any(c is not None for c in cur):
        appends, ends, restarts = [], [], []
        for s in range(B):
            if cur[s] is None:
                continue
            n = min(int(rng.choice(chunks)), lens[cur[s]] - pos[s])
            appends.append((s, cur[s], pos[s], pos[s] + n))
            pos[s] += n
            if pos[s] == lens[cur[s]]:
                ends.append(s)
        for s in ends:
            nxt = queue.pop(0) if queue else None
            restarts.append((s, cur[s], nxt))
            cur[s], pos[s] = nxt, 0
        rounds.append((appends, ends, restarts))
    return rounds


def append_host(b, stype, mono, s, x):
    """x: [2, n] of the batch's sample type, through the entry point the type is named after"""
    if stype == PCM_S16:
        b.append(s, np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1]))
    elif mono:
        b.append_input(s, np.ascontiguousarray(x[0]))
    else:
        b.append_input(s, np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1]))


def get_state(b, s):
    n = b.lib.lamehip_abi_sizeof(4)
    buf = C.create_string_buffer(n)
    assert b.lib.lamehip_batch_get_state(b.b, s, buf, n) == n
    return buf.raw


class Turnover:
    """what carrying out a schedule left: per utterance the concatenated drains, the tag frame handed out right behind the
    ending round, the frame count; per round what the hooks recorded"""

    def __init__(self):
        self.bytes, self.tags, self.frames, self.ending_rounds = {}, {}, {}, []


def run_schedule(b, stype, mono, xs, rounds, tagging, before_round=None, after_round=None, in_gap=None, append=None):
    """append, end, round, drain + tag, restart.  before_round(r) / after_round(r): hooks around encode_available();
    in_gap(r, restarts): behind the round's drains and in front of its restarts; append(s, x): another way to feed."""
    res = Turnover()
    for r, (appends, ends, restarts) in enumerate(rounds):
        for s, u, a, e in appends:
            (append or (lambda s, x: append_host(b, stype, mono, s, x)))(s, xs[u][:, a:e])
            res.bytes.setdefault(u, b"")
        for s in ends:
            assert b.stream_ended(s) is False
            b.end_stream(s)
            assert b.stream_ended(s) is False       # (it ends with the round, not with the call)
        if before_round:
            before_round(r)
        b.encode_available()
        if after_round:
            after_round(r)
        if ends:
            res.ending_rounds.append(r)
        for s, u, a, e in appends:
            res.bytes[u] += b.drain(s)
            assert b.stream_ended(s) is (s in ends)
            if s in ends:
                res.frames[u] = b.frames(s)
                if tagging:
                    res.tags[u] = b.tag(s)
            elif tagging:
                with pytest.raises(RuntimeError, match="lamehip_batch_tag_ptr: .*lamehip_batch_finish"):
                    b.tag(s)
        if in_gap:
            in_gap(r, restarts)
        for s, u, nxt in restarts:
            b.restart_stream(s)
            assert b.stream_ended(s) is False and b.frames(s) == 0
    return res


def one_shot(enc, stype, mono, xs, cap):
    """(audio bytes, file images) of a whole-stream batch of the same samples, packed and tagged on the device"""
    b = lamehip.Batch(enc, len(xs), cap)
    b.set_device_packing()
    b.set_device_tagging()
    if stype != PCM_S16:
        b.set_sample_type(stype)
    for s, x in enumerate(xs):
        if stype == PCM_S16:
            b.set_pcm(s, x[0], x[1])
        elif mono:
            b.set_input(s, x[0])
        else:
            b.set_input(s, x[0], x[1])
    b.encode()
    out = [b.get_bytes(s) for s in range(len(xs))], [b.get_bytes_tagged(s) for s in range(len(xs))]
    b.close()
    return out


def check_turnover(res, T, audio, images, tagging, what=""):
    """every utterance's drains are its one-shot bytes; with tags: the tag is the one-shot image's head, and T zeros + drains
    with the tag written over the head are the whole image"""
    assert sorted(res.bytes) == list(range(len(audio))), what
    for u, want in enumerate(audio):
        assert res.bytes[u] == want, "%s: bytes of utterance %d" % (what, u)
        assert res.frames[u] > 0
        if tagging:
            assert len(res.tags[u]) == T and res.tags[u] == images[u][:T], "%s: tag of utterance %d" % (what, u)
            whole = bytearray(T) + res.bytes[u]
            whole[:T] = res.tags[u]
            assert bytes(whole) == images[u], "%s: image of utterance %d" % (what, u)
