"""The slots of an incremental batch (lamehip_batch_end_stream / _restart_stream) without a device: the SOURCE of the restart
kernel (csrc/lh_slots.hip) run by the fiber emulator of tests/hipemu against numpy -- listed slots back at the initial image or
zero, every other byte untouched --, and the two kernels that now take "behind the flush" per stream (csrc/lh_drain.hip:
lh_drain_pos_kernel, csrc/lh_tag.hip: lh_tag_resume_kernel) over two streams of which one ends in the round and one does not.
Every check is byte or integer equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers
import lamehip
from lamehip.types import LhFrameOut
from test_emulator import LhStreamDesc
from test_incremental_packing import (LhDrainParams, LhDrainRow, OFF_CURSOR, OFF_NEXT, aligned, drain_params, parse_frames,
                                      tiles_of)
from test_incremental_tag import LhTagCarry, LhTagPow
from test_device_tag import settings

SLOTS_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_slots")
EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu")
GUARD = 256
SYMBOLS = ["lamehip_batch_end_stream", "lamehip_batch_stream_ended", "lamehip_batch_restart_stream", "lamehip_batch_last_restart_ms"]


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_slots.so"], SLOTS_DIR)
    e = C.CDLL(os.path.join(SLOTS_DIR, "libhipemu_slots.so"))
    e.lh_emu_slot_restart.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    e.lh_emu_slot_sizeof.argtypes = [C.c_int]
    e.lh_emu_drain.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    e.lh_emu_drain_tiles.restype = C.c_longlong
    e.lh_emu_drain_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    e.lh_emu_drain_bound.restype = C.c_longlong
    e.lh_emu_drain_bound.argtypes = [C.c_longlong] * 5
    e.lh_emu_tag_resume_slots.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 12 + [C.c_int, C.c_void_p]
    e.lh_emu_tag_resume.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 12 + [C.c_int]
    return e


@pytest.fixture(scope="module")
def emu_encode():
    helpers.locked_make([], EMU_DIR)
    return C.CDLL(os.path.join(EMU_DIR, "libhipemu_lame.so"))


# ---- the restart kernel ----

class Records:
    """one array of B records of `size' bytes between guards, the first record `lead' bytes behind a 16-byte boundary, every
    byte poisoned"""

    def __init__(self, B, size, poison, lead=0):
        self.B, self.size = B, size
        self.raw = np.empty(GUARD + B * size + GUARD + 32, np.uint8)
        self.at = GUARD + (lead - (self.raw.ctypes.data + GUARD)) % 16
        self.raw[:] = poison
        self.before = self.raw.copy()

    def addr(self):
        return self.raw.ctypes.data + self.at

    def fill(self, rng):
        self.raw[self.at:self.at + self.B * self.size] = rng.integers(1, 256, self.B * self.size, dtype=np.uint8)
        self.before = self.raw.copy()

    def expect(self, listed, image=None):
        want = self.before.copy()
        for s in listed:
            lo = self.at + s * self.size
            want[lo:lo + self.size] = 0 if image is None else image[s * self.size:(s + 1) * self.size]
        return want


def slot_lists(B):
    lists = {"first": [0], "last": [B - 1], "neighbours": [B // 2, min(B // 2 + 1, B - 1)] if B > 1 else [0],
             "every-second": list(range(0, B, 2)), "all": list(range(B)), "empty": []}
    return {k: sorted(set(v)) for k, v in lists.items()}


@pytest.mark.parametrize("absent", [None, "drain", "tag", "gain", "state"])
@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_restart_kernel_matches_numpy(B, absent, emu):
    """Batches of 1, 3, 70 and 300 streams (across a wave's and a workgroup's worth of workgroups), every record array
    poisoned between guards, the real record sizes of this build (sizeof(LhStreamState) is what decides the tail path): after
    the launch the listed slots hold the initial image (LhStreamState) or zeros (the carries), every other byte, guards
    included, is what it was.  Each optional record absent in turn; the list in an order of its own."""
    sizes = [emu.lh_emu_slot_sizeof(k) for k in range(4)]
    assert sizes[0] == lamehip.load_library().lamehip_abi_sizeof(4) and sizes[1] == 8 and sizes[2] == C.sizeof(LhTagCarry)
    assert sizes[3] > 0
    rng = np.random.default_rng(7100 + B)
    for name, listed in slot_lists(B).items():
        state = Records(B, sizes[0], 0xA5)
        image = Records(B, sizes[0], 0x3C)
        carries = {"drain": Records(B, sizes[1], 0x5A), "tag": Records(B, sizes[2], 0x6B), "gain": Records(B, sizes[3], 0x7C)}
        for r in [state, image] + list(carries.values()):
            r.fill(rng)
        img = image.raw[image.at:image.at + B * sizes[0]].copy()
        order = np.array(listed, dtype=np.int32)[::-1].copy() if listed else np.zeros(1, np.int32)
        ptr = lambda key: None if absent == key else carries[key].addr()
        assert emu.lh_emu_slot_restart(order.ctypes.data, len(listed), B, None if absent == "state" else state.addr(), image.addr(),
                                       ptr("drain"), ptr("tag"), ptr("gain")) == 0
        assert np.array_equal(state.raw, state.expect([] if absent == "state" else listed, img)), (name, "state")
        assert np.array_equal(image.raw, image.before), (name, "the image was written")
        for key, r in carries.items():
            assert np.array_equal(r.raw, r.expect([] if absent == key else listed)), (name, key)


def test_restart_kernel_off_boundary_and_bad_entries(emu):
    """Records whose arrays start off a 16-byte boundary, and differently far off it for the states and their image (the
    copy then goes byte by byte); entries outside [0, B) are skipped"""
    sizes = [emu.lh_emu_slot_sizeof(k) for k in range(4)]
    rng = np.random.default_rng(7777)
    B = 5
    for lead_state, lead_image in [(8, 8), (4, 12), (1, 0)]:
        state, image = Records(B, sizes[0], 0xA5, lead_state), Records(B, sizes[0], 0x3C, lead_image)
        tag = Records(B, sizes[2], 0x6B, 4)
        for r in (state, image, tag):
            r.fill(rng)
        img = image.raw[image.at:image.at + B * sizes[0]].copy()
        order = np.array([3, -1, B, 1, 1 << 20], dtype=np.int32)
        assert emu.lh_emu_slot_restart(order.ctypes.data, len(order), B, state.addr(), image.addr(), None, tag.addr(), None) == 0
        assert np.array_equal(state.raw, state.expect([1, 3], img))
        assert np.array_equal(tag.raw, tag.expect([1, 3]))


# ---- the drain with finality per stream ----

def test_drain_takes_the_flush_per_stream(emu, emu_encode):
    """Two streams through the encode kernel's source with the device packer: stream 0 is the fixture, whole, and ends in the
    second round; stream 1 is the same signal and goes on.  The scalar `final' is 0 throughout.  Stream 0's P is the end of its
    last frame -- all of the fixture's bytes come out --, stream 1's is what the walk gives for it alone.  In a round without
    frames the ended stream reports the same P: the undrained count before its drain, 0 after it."""
    g, pcm = helpers.load_golden("vbr2_js_44k")
    enc = lamehip.Encoder(require_device=False, **helpers.golden_encoder_kwargs(g))
    cfg, tab, lib = enc.config(), enc.tables(), enc.lib
    nframes = int(g["nframes"])
    want = g["mp3"].tobytes()
    frames = parse_frames(want, cfg)
    n = pcm.shape[1]
    pcm_pool = np.concatenate([pcm[0], pcm[1]]).astype(np.int16)
    size = emu.lh_emu_slot_sizeof(0)
    cap = nframes * 1500
    states = aligned(2 * size, 0)
    for s in range(2):
        lib.lh_state_init(C.c_void_p(states.ctypes.data + s * size), C.byref(cfg))
    out = aligned(2 * cap + 64, 0)
    got = [(LhFrameOut * nframes)(), (LhFrameOut * nframes)()]
    cut0, cut1 = nframes - 3, 3                     # round 1: stream 0's frames [0, cut0), stream 1's [0, cut1)
    rounds = [((0, cut0, 0), (0, cut1, 0)), ((cut0, nframes, 1), (cut1, cut1 + 2, 0)), ((nframes, nframes, 1), (cut1 + 2, cut1 + 2, 0))]
    drained = np.zeros(2, np.int64)
    carry = np.zeros(2, np.int64)
    frame_max = max(f[1] for f in frames)
    p = drain_params(cfg, lib, 0)
    collected = b""
    for r, per_stream in enumerate(rounds):
        descs = (LhStreamDesc * 2)()
        for s, (lo, hi, flush) in enumerate(per_stream):
            descs[s] = LhStreamDesc(0, n, 0, n, 0, lo, hi, s * cap, cap, flush, 0)
            if hi > lo:
                emu_encode.lh_emu_encode_bytes(C.byref(cfg), C.byref(tab), pcm_pool.ctypes.data_as(C.c_void_p), C.byref(descs[s]),
                                               C.c_void_p(states.ctypes.data + s * size), got[s], out.ctypes.data_as(C.c_void_p), 1)
        # what the existing walk gives for stream 1, alone, from a copy of its carry
        alone_carry, alone_rows = carry[1:2].copy(), (LhDrainRow * 2)()
        tiles, ntiles, padded = tiles_of(emu, [cap])
        buf = aligned(padded + 32, 0xA5)
        assert emu.lh_emu_drain(C.byref(p), C.byref(descs[1]), states.ctypes.data + size, drained[1:2].copy().ctypes.data,
                                alone_carry.ctypes.data, out.ctypes.data, alone_rows, 1, tiles, ntiles, buf.ctypes.data, padded) == 0
        # the round's drain over both
        tiles, ntiles, padded = tiles_of(emu, [cap, cap])
        buf = aligned(padded + 32, 0xA5)
        rows = (LhDrainRow * 3)()
        assert emu.lh_emu_drain(C.byref(p), descs, states.ctypes.data, drained.ctypes.data, carry.ctypes.data, out.ctypes.data, rows, 2,
                                tiles, ntiles, buf.ctypes.data, padded) == 0
        assert rows[0].status == 0 and rows[1].status == 0
        assert (rows[1].upto, rows[1].n, carry[1]) == (alone_rows[0].upto, alone_rows[0].n, alone_carry[0]), r
        cursor1 = int(np.frombuffer(states[size + OFF_CURSOR:size + OFF_CURSOR + 8].tobytes(), np.int64)[0])
        assert rows[1].upto in (cursor1, cursor1 - cfg.sideinfo_len)
        if r == 0:
            # (not ending yet: in front of the end of its frames so far, the reservoir's bytes are not final)
            next0 = int(np.frombuffer(states[OFF_NEXT:OFF_NEXT + 8].tobytes(), np.int64)[0])
            assert rows[0].upto <= next0 == frames[cut0 - 1][0] + frames[cut0 - 1][1]
            collected += buf[rows[0].off:rows[0].off + rows[0].n].tobytes()
            drained[0] += rows[0].n
        else:
            assert rows[0].upto == len(want) == rows[0].next, r
            if r == 1:
                # the ended stream is left undrained: the next round must find the same bytes again
                assert rows[0].n == len(want) - drained[0] > 0
                undrained = buf[rows[0].off:rows[0].off + rows[0].n].tobytes()
            else:
                assert rows[0].n == len(want) - drained[0] and buf[rows[0].off:rows[0].off + rows[0].n].tobytes() == undrained
                collected += undrained
                drained[0] += rows[0].n
                # ... and, drained, nothing
                rows2 = (LhDrainRow * 3)()
                assert emu.lh_emu_drain(C.byref(p), descs, states.ctypes.data, drained.ctypes.data, carry.ctypes.data, out.ctypes.data,
                                        rows2, 2, tiles, ntiles, buf.ctypes.data, padded) == 0
                assert (rows2[0].upto, rows2[0].n, rows2[0].status) == (len(want), 0, 0)
        drained[1] += rows[1].n
    assert collected == want
    assert drained[1] <= frames[cut1 + 1][0] + frames[cut1 + 1][1]       # (stream 1 is in the middle of its stream)
    assert frame_max > 0
    enc.close()


# ---- the tag kernel with finality per stream ----

def tag_round(emu, p, pw, tmpl, pool, base, cap, upto, idx, padding, ext, carries, tags, final, flush=None):
    arr = lambda t, x: np.ascontiguousarray(np.array(x, dtype=t))
    B = len(base)
    zero = [0] * B
    a_upto, a_base, a_cap = arr(np.int64, upto), arr(np.int64, base), arr(np.int64, cap)
    a_st, a_rst = arr(np.int32, zero), arr(np.int32, zero)
    a_nf, a_pad, a_ext = arr(np.int32, [len(x) for x in idx]), arr(np.int32, padding), arr(np.int32, ext)
    a_idx = arr(np.int8, [i for x in idx for i in x] + [0])
    args = [C.byref(p), C.byref(pw), tmpl, B, a_upto.ctypes.data, a_st.ctypes.data, a_rst.ctypes.data, a_nf.ctypes.data, a_pad.ctypes.data,
            a_ext.ctypes.data, a_idx.ctypes.data, a_base.ctypes.data, a_cap.ctypes.data, pool.ctypes.data, carries.ctypes.data,
            tags.ctypes.data, 1 if final else 0]
    if flush is None:
        assert emu.lh_emu_tag_resume(*args) == 0
    else:
        a_flush = arr(np.int32, flush)
        assert emu.lh_emu_tag_resume_slots(*(args + [a_flush.ctypes.data])) == 0


def test_tag_resume_takes_the_flush_per_stream(emu):
    """Two streams over three rounds of random bytes and bit rates; in the last round stream 0 ends (its descriptor says flush)
    and stream 1 does not, scalar `final' 0.  Stream 0's frame is the one the scalar-final launch makes for it from the same
    carry; stream 1's tag row stays at its poison and its carry moves on exactly as in a round that is not final.  A later
    round in which the ended stream keeps the flag without frames leaves its row and carry alone."""
    lib = lamehip.load_library()
    lib.lh_tag_template.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.lh_tag_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lh_tag_pow_table.argtypes = [C.c_void_p]
    enc, cfg, v, p, tmpl = settings(lib, dict(vbr_q=2))
    pw = LhTagPow()
    lib.lh_tag_pow_table(C.byref(pw))
    rng = np.random.default_rng(5150)
    csz = C.sizeof(LhTagCarry)
    cap = 40000
    pool = aligned(2 * cap + 64, 0)
    pool[:] = rng.integers(0, 256, len(pool), dtype=np.uint8)
    base = [16, 16 + cap + 5]
    lo, hi = cfg.vbr_min_bitrate_index, cfg.vbr_max_bitrate_index
    carries = aligned(2 * csz, 0)
    tags = np.full(2 * p.total, 0x5A, np.uint8)
    upto = [0, 0]
    for r in range(2):
        idx = [[int(i) for i in rng.integers(lo, hi + 1, 7 + r)] for s in range(2)]
        upto = [upto[s] + 3000 + 17 * s + r for s in range(2)]
        tag_round(emu, p, pw, tmpl, pool, base, [cap, cap], upto, idx, [0, 0], [1, 2], carries, tags, False, [0, 0])
        assert (tags == 0x5A).all()
    saved = carries.copy()
    idx = [[int(i) for i in rng.integers(lo, hi + 1, 5)] for s in range(2)]
    upto = [upto[0] + 4001, upto[1] + 2222]
    pad = [777, 555]
    # the references: the scalar-final launch, and a round that is not final, from the same carries
    ref_carry, ref_tags = saved.copy(), np.full(2 * p.total, 0x5A, np.uint8)
    tag_round(emu, p, pw, tmpl, pool, base, [cap, cap], upto, idx, pad, [2, 1], ref_carry, ref_tags, True)
    plain_carry, plain_tags = saved.copy(), np.full(2 * p.total, 0x5A, np.uint8)
    tag_round(emu, p, pw, tmpl, pool, base, [cap, cap], upto, idx, pad, [2, 1], plain_carry, plain_tags, False)
    assert (plain_tags == 0x5A).all() and ref_tags[:p.total].any()
    # per stream
    tag_round(emu, p, pw, tmpl, pool, base, [cap, cap], upto, idx, [pad[0], -123456], [2, 1], carries, tags, False, [1, 0])
    assert np.array_equal(tags[:p.total], ref_tags[:p.total])
    assert (tags[p.total:] == 0x5A).all()
    assert np.array_equal(carries[:csz], ref_carry[:csz])
    assert np.array_equal(carries[csz:], plain_carry[csz:])
    # the ended stream in a later round: the flag, no frames, the same position
    before_c, before_t = carries[:csz].copy(), tags.copy()
    idx = [[], [int(i) for i in rng.integers(lo, hi + 1, 4)]]
    upto = [upto[0], upto[1] + 900]
    tag_round(emu, p, pw, tmpl, pool, base, [cap, cap], upto, idx, [-1, -1], [0, 3], carries, tags, False, [1, 0])
    assert np.array_equal(carries[:csz], before_c) and np.array_equal(tags, before_t)
    assert LhTagCarry.from_buffer_copy(bytes(carries[csz:])).frames == 7 + 8 + 5 + 4
    enc.close()


# ---- symbols ----

def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(helpers.ROOT, "include", "lamehip.h")).read()
    lib = lamehip.load_library()
    for name in SYMBOLS:
        assert re.search(r"^(int|float)\s+%s\(lamehip_batch \*" % name, header, re.M), name
        assert getattr(lib, name) is not None
    for method in ("end_stream", "stream_ended", "restart_stream", "restart_ms"):
        assert callable(getattr(lamehip.Batch, method))
