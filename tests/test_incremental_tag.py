"""The tag frames of an incremental batch that packs on the device (lamehip_batch_set_incremental_tagging) without a device:
the SOURCE of lh_tag_resume_kernel (csrc/lh_tag.hip) run by the fiber emulator of tests/hipemu round after round, its carry
(csrc/lh_tag.h: LhTagCarry) against the host's bookkeeping driven over the whole stream (csrc/lh_vbrtag.c: lh_tag_crc,
lh_tag_add_frame, lh_tag_frame) -- the CRC after every round, the bag after every round, the final frame, which is also the
one-shot kernel's and, where the compiled reference is there, the reference's lame_get_lametag_frame --; the table of
advances by powers of two; the host side as a stand-alone program under AddressSanitizer and UBSan.  Every check is byte or
integer equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import lamehip
import test_device_tag as tdt
from test_device_tag import CONFIGS, LhVbrTag, host_crc, host_frame, settings

INC_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_tag_inc")
NPOW = 40                                       # LH_TAG_NPOW (csrc/lh_tag.h)


class LhTagCarry(C.Structure):
    _fields_ = [("crc_upto", C.c_longlong), ("crc", C.c_uint32), ("frames", C.c_int), ("want", C.c_int), ("pos", C.c_int),
                ("sum", C.c_int), ("mode_ext", C.c_int), ("bad", C.c_int), ("pad", C.c_int), ("bag", C.c_int * 400)]


class LhTagPow(C.Structure):
    _fields_ = [("col", (C.c_uint16 * 16) * NPOW)]


@pytest.fixture(scope="module")
def lib():
    lib = lamehip.load_library()
    lib.lh_tag_crc.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.lh_tag_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    lib.lh_tag_template.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.lh_tag_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lh_tag_pow_table.argtypes = [C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_tag_inc.so"], INC_DIR)
    e = C.CDLL(os.path.join(INC_DIR, "libhipemu_tag_inc.so"))
    e.lh_emu_tag_resume.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 12 + [C.c_int]
    e.lh_emu_tag.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 9
    e.lh_emu_tag_advance_by.argtypes = [C.c_uint, C.c_void_p, C.c_longlong]
    e.lh_emu_tag_advance_by.restype = C.c_uint
    assert e.lh_emu_tag_sizeof_carry() == C.sizeof(LhTagCarry)
    return e


@pytest.fixture(scope="module")
def pow_table(lib):
    pw = LhTagPow()
    lib.lh_tag_pow_table(C.byref(pw))
    return pw


@pytest.fixture(scope="module")
def params(lib):
    enc, cfg, v, p, tmpl = settings(lib, dict(brate=128))
    enc.close()
    return p, tmpl


GUARD = 256


class Rounds:
    """B streams' carries and tag rows between canaries, and lh_tag_resume_kernel over them round by round"""

    def __init__(self, emu, p, pw, tmpl, B):
        self.emu, self.p, self.pw, self.tmpl, self.B = emu, p, pw, tmpl, B
        self.csz = C.sizeof(LhTagCarry)
        self.craw = np.full(GUARD + B * self.csz + GUARD + 8, 0x5A, np.uint8)
        self.c0 = GUARD + (-(self.craw.ctypes.data + GUARD)) % 8
        self.craw[self.c0:self.c0 + B * self.csz] = 0
        self.traw = np.full(GUARD + B * p.total + GUARD, 0x5A, np.uint8)

    def carry(self, s):
        return LhTagCarry.from_buffer_copy(bytes(self.craw[self.c0 + s * self.csz:self.c0 + (s + 1) * self.csz]))

    def carries(self):
        return self.craw[self.c0:self.c0 + self.B * self.csz].copy()

    def set_carries(self, saved):
        self.craw[self.c0:self.c0 + self.B * self.csz] = saved

    def tag(self, s):
        return bytes(self.traw[GUARD + s * self.p.total:GUARD + (s + 1) * self.p.total])

    def run(self, pool, base, cap, upto, idx, status=None, row_status=None, padding=None, ext=None, final=False):
        """one round: stream s's slice starts at pool[base[s]], upto[s] bytes of it are final, idx[s] are the round's
        bit-rate indices; the pool must come back unchanged, and so must everything around the carries and the tag rows
        (the rows themselves too unless the round is final)"""
        B = self.B
        arr = lambda t, x: np.ascontiguousarray(np.array(x, dtype=t))
        zero = [0] * B
        a_upto, a_base, a_cap = arr(np.int64, upto), arr(np.int64, base), arr(np.int64, cap)
        a_st, a_rst = arr(np.int32, status or zero), arr(np.int32, row_status or zero)
        a_nf, a_pad, a_ext = arr(np.int32, [len(x) for x in idx]), arr(np.int32, padding or zero), arr(np.int32, ext or zero)
        a_idx = arr(np.int8, [i for x in idx for i in x] + [0])
        pool_before, tags_before = pool.copy(), self.traw.copy()
        assert self.emu.lh_emu_tag_resume(C.byref(self.p), C.byref(self.pw), self.tmpl, B, a_upto.ctypes.data, a_st.ctypes.data,
                                          a_rst.ctypes.data, a_nf.ctypes.data, a_pad.ctypes.data, a_ext.ctypes.data, a_idx.ctypes.data,
                                          a_base.ctypes.data, a_cap.ctypes.data, pool.ctypes.data, self.craw.ctypes.data + self.c0,
                                          self.traw.ctypes.data + GUARD, 1 if final else 0) == 0
        assert (pool == pool_before).all(), "the kernel wrote into the byte pool"
        assert (self.craw[:self.c0] == 0x5A).all() and (self.craw[self.c0 + B * self.csz:] == 0x5A).all(), "wrote around the carries"
        assert (self.traw[:GUARD] == 0x5A).all() and (self.traw[GUARD + B * self.p.total:] == 0x5A).all(), "wrote around the tag rows"
        if not final:
            assert (self.traw == tags_before).all(), "a round that is not final wrote a tag row"


ROUND_LENGTHS = [0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8193]


@pytest.mark.parametrize("offset", [0, 1, 7, 2881])
def test_crc_continues_over_rounds(offset, lib, emu, params, pow_table):
    """random bytes cut into rounds of every length at which the CRC kernel takes another path, in several orders, the
    slice `offset' bytes behind a 16-byte boundary: after every round the carried CRC is the host CRC of the prefix.  The
    bytes around the slice are canaries, none zero, and so is everything at and behind P: a read there changes the result
    -- the round is run twice from the same carry with different bytes behind P --, and a write shows."""
    p, tmpl = params
    rng = np.random.default_rng(2000 + offset)
    guard = 4096
    for order in range(4):
        plan = [ROUND_LENGTHS[(r * (order + 1) + order) % 13] for r in range(13)] if order < 3 else list(rng.permutation(ROUND_LENGTHS))
        total = int(sum(plan))
        raw = np.empty(guard + offset + total + guard + 16, np.uint8)
        lead = (-raw.ctypes.data) % 16
        pool = raw[lead:]
        pool[:] = rng.integers(1, 256, len(pool), dtype=np.uint8)
        at = guard + offset
        assert (pool.ctypes.data + at) % 16 == offset % 16
        data = rng.integers(0, 256, total, dtype=np.uint8)
        cap = total + 100
        rr = Rounds(emu, p, pow_table, tmpl, 1)
        upto = 0
        for n in plan:
            upto += int(n)
            pool[at:at + upto] = data[:upto]
            saved = rr.carries()
            pool[at + upto:at + cap] = 0xEE
            rr.run(pool, [at], [cap], [upto], [[]])
            first = rr.carries()
            rr.set_carries(saved)
            pool[at + upto:at + cap] = rng.integers(1, 256, cap - upto, dtype=np.uint8)
            rr.run(pool, [at], [cap], [upto], [[]])
            assert (rr.carries() == first).all(), (offset, order, upto)
            c = rr.carry(0)
            assert c.crc_upto == upto and c.bad == 0
            assert c.crc == host_crc(lib, data[:upto]), (offset, order, upto)
            assert (c.frames, c.pos, c.sum) == (0, 0, 0)


BAG_PLANS = [
    [0, 1, 255, 256, 257, 31, 0, 300, 500, 150],        # 512: over 400 inside a round; 800 and 1600 exactly at a round's end
    [399, 1, 1, 500, 800],                              # 400 exactly at a round's end; over 800 and over 1600 inside a round
    [1, 1700],                                          # from 1 frame to 1701: two halvings at once
    [1701],
    [256, 256, 256, 256, 256, 256, 256],
]


@pytest.mark.parametrize("plan", range(len(BAG_PLANS)), ids=["-".join(str(n) for n in pl) for pl in BAG_PLANS])
def test_bag_carries_over_rounds(plan, lib, emu, params, pow_table):
    """after every round the carry's fill, sampling distance, sum and samples are those of an LhVbrTag fed the same frames
    one by one"""
    p, tmpl = params
    rng = np.random.default_rng(3000 + plan)
    v = LhVbrTag()
    v.want, v.size = 1, 400             # (lh_tag_init's)
    rr = Rounds(emu, p, pow_table, tmpl, 1)
    pool = np.full(64, 0x77, np.uint8)
    total = 0
    for n in BAG_PLANS[plan]:
        idx = [int(i) for i in rng.integers(1, 15, n)]
        for i in idx:
            lib.lh_tag_add_frame(C.byref(v), int(p.kbps[i]))
        rr.run(pool, [8], [0], [0], [idx], ext=[n % 4])
        total += n
        c = rr.carry(0)
        assert (c.frames, c.pos, c.sum, c.bad) == (total, v.pos, v.sum, 0), (n, total)
        assert c.want == v.want or total == 0
        assert list(c.bag[:c.pos]) == list(v.bag[:v.pos]), (n, total)
        if n:
            assert c.mode_ext == n % 4
    assert total in (1701, 1750, 1792) and v.want == 8


def cut(rng, total, rounds):
    """`total' cut into `rounds' parts, empty ones allowed"""
    at = sorted(int(x) for x in rng.integers(0, total + 1, rounds - 1))
    return [b - a for a, b in zip([0] + at, at + [total])]


def run_streams(emu, p, pw, tmpl, rng, streams, rounds, gap=37):
    """lh_tag_resume_kernel over `streams' [(audio bytes, status, bit-rate indices, padding, idle)] in `rounds' rounds: every
    stream's bytes and frames are cut at random places (an idle stream gets nothing in the odd rounds; a status shows from the
    second round on, in the packer's state or in the drain's row), the last round is the final one.  Returns (tag rows, the
    mode extension of each stream's last frame)."""
    B = len(streams)
    base, cap, at = [], [], 5
    for (audio, status, idx, pad, idle) in streams:
        base.append(at)
        cap.append(len(audio) + 11)
        at += len(audio) + 11 + gap
    pool = np.full(at + 64, 0xA5, np.uint8)
    rr = Rounds(emu, p, pw, tmpl, B)
    cuts_b, cuts_f = [], []
    for (audio, status, idx, pad, idle) in streams:
        live = [r for r in range(rounds) if not (idle and r % 2 == 1 and r != rounds - 1)]
        cb, cf = [0] * rounds, [0] * rounds
        for r, nb, nf in zip(live, cut(rng, len(audio), len(live)), cut(rng, len(idx), len(live))):
            cb[r], cf[r] = nb, nf
        cuts_b.append(cb)
        cuts_f.append(cf)
    upto, fpos, last_ext = [0] * B, [0] * B, [0] * B
    for r in range(rounds):
        idx_r, ext_r, st, rst = [], [], [], []
        for s, (audio, status, idx, pad, idle) in enumerate(streams):
            upto[s] += cuts_b[s][r]
            pool[base[s]:base[s] + upto[s]] = np.frombuffer(audio[:upto[s]], np.uint8)
            pool[base[s] + upto[s]:base[s] + cap[s]] = 0xC3 + r         # (behind P: not final)
            idx_r.append(idx[fpos[s]:fpos[s] + cuts_f[s][r]])
            fpos[s] += cuts_f[s][r]
            e = int(rng.integers(0, 4))
            ext_r.append(e)
            if cuts_f[s][r]:
                last_ext[s] = e
            on = status and (r >= 1 or rounds == 1)
            st.append(status if on and s % 2 == 0 else 0)
            rst.append(status | 16 if on and s % 2 == 1 else 0)
        rr.run(pool, base, cap, upto, idx_r, status=st, row_status=rst, padding=[x[3] for x in streams], ext=ext_r,
               final=(r == rounds - 1))
    return [rr.tag(s) for s in range(B)], last_ext


def one_shot(emu, p, tmpl, streams, exts):
    """the one-shot lh_tag_kernel of the same library over the same bytes and frames"""
    emu_like = emu
    return tdt.run_kernel(emu_like, p, tmpl, [(a, st, idx, pad, exts[s]) for s, (a, st, idx, pad, idle) in enumerate(streams)])


@pytest.mark.parametrize("name,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_final_frame_matches_lh_tag_frame_and_the_one_shot_kernel(name, kw, lib, emu, pow_table):
    """streams of 1, 2, 401 and 1700 frames with random bit rates of the setting's range and random bytes, cut into 1 to 7
    rounds, one stream idle in some rounds, one with a status (packer's or drain's), one without frames: the final round's
    tag row is lh_tag_frame's frame and the one-shot kernel's; the status and the empty stream get zeros; nothing outside
    the carries and the tag rows is written"""
    enc, cfg, v0, p, tmpl = settings(lib, kw)
    k = [c[0] for c in CONFIGS].index(name)
    rng = np.random.default_rng(len(name) * 137 + p.total)
    lo, hi = (cfg.bitrate_index,) * 2 if cfg.vbr == 0 else (cfg.vbr_min_bitrate_index, cfg.vbr_max_bitrate_index)
    for rounds in sorted({1 + k % 7, 1 + (k + 3) % 7, 7 if k == 0 else 1 + (k + 5) % 7}):
        streams = []
        for s, nf in enumerate([1, 0, 2, 401, 7, 1700, 30, 9]):
            audio = rng.integers(0, 256, 0 if nf == 0 else int(rng.integers(1, 9000)) + 16 * s, dtype=np.uint8).tobytes()
            idx = [int(i) for i in rng.integers(lo, hi + 1, nf)]
            streams.append((audio, 3 if nf in (7, 9) else 0, idx, int(rng.integers(0, 2400)), nf == 30))
        tags, exts = run_streams(emu, p, pow_table, tmpl, rng, streams, rounds)
        shot = one_shot(emu, p, tmpl, streams, exts)
        for s, (audio, status, idx, pad, idle) in enumerate(streams):
            want = host_frame(lib, cfg, v0, audio, idx, pad, exts[s])
            if status or not idx:
                assert want is None or status
                assert tags[s] == bytes(p.total), (name, rounds, s)
            else:
                assert tags[s] == want, (name, rounds, s)
            assert tags[s] == shot[s], (name, rounds, s)
    enc.close()


def test_a_position_that_goes_back_or_out_of_the_slice_makes_no_tag(lib, emu, params, pow_table):
    """a round whose position lies in front of the bytes already covered, or behind the slice's end, marks the stream: zeros
    at the end, whatever follows; its neighbour is untouched by it"""
    p, tmpl = params
    rng = np.random.default_rng(77)
    audio = rng.integers(0, 256, 3000, dtype=np.uint8)
    pool = np.full(8000, 0xA5, np.uint8)
    base, cap = [16, 4016], [3000, 3000]
    for s in range(2):
        pool[base[s]:base[s] + 3000] = audio
    for kind in ("back", "out"):
        rr = Rounds(emu, p, pow_table, tmpl, 2)
        rr.run(pool, base, cap, [1000, 1000], [[9] * 3, [9] * 3])
        rr.run(pool, base, cap, [999 if kind == "back" else 3001, 2000], [[9], [9]])
        assert rr.carry(0).bad == 1 and rr.carry(1).bad == 0
        rr.run(pool, base, cap, [3000, 3000], [[9], [9]], padding=[700, 700], ext=[2, 2], final=True)
        assert rr.tag(0) == bytes(p.total)
        assert rr.tag(1)[:2] == b"\xff\xfb" and rr.carry(1).crc == host_crc(lib, audio)


def test_advance_table(lib, emu, pow_table):
    """the table of advances by powers of two: k up to 16 against the host CRC stepped from every unit vector over 1 << k
    zeros; every larger k against the one before applied twice; runs of any length through the set bits"""
    zeros = bytes(1 << 16)
    for k in range(17):
        for j in range(16):
            v = LhVbrTag()
            v.music_crc = 1 << j
            lib.lh_tag_crc(C.byref(v), zeros, 1 << k)
            assert pow_table.col[k][j] == v.music_crc, (k, j)
    rng = np.random.default_rng(4)
    for k in range(17, NPOW):
        for crc in [1 << j for j in range(16)] + [int(x) for x in rng.integers(0, 65536, 8)]:
            half = emu.lh_emu_tag_advance_by(crc, C.byref(pow_table), 1 << (k - 1))
            assert emu.lh_emu_tag_advance_by(crc, C.byref(pow_table), 1 << k) == emu.lh_emu_tag_advance_by(half, C.byref(pow_table), 1 << (k - 1))
    for n in [0, 1, 3, 255, 256, 65535, 65537] + [int(x) for x in rng.integers(0, 1 << 20, 6)]:
        v = LhVbrTag()
        v.music_crc = 0xBEEF
        lib.lh_tag_crc(C.byref(v), bytes(n), n)
        assert emu.lh_emu_tag_advance_by(0xBEEF, C.byref(pow_table), n) == v.music_crc, n


REF_CONFIGS = [c for c in CONFIGS]


@pytest.mark.skipif(not helpers.have_reference(), reason="needs oracle/_ref (reference sources)")
@pytest.mark.parametrize("name,kw", REF_CONFIGS, ids=[c[0] for c in REF_CONFIGS])
def test_final_frame_matches_reference(name, kw, lib, emu, pow_table):
    """the reference's own audio bytes cut at arbitrary byte positions and the oracle's frames cut at arbitrary frame
    positions, through the kernel round by round: the final tag row is the reference's lame_get_lametag_frame"""
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
    rng = np.random.default_rng(len(name))
    rounds = 5
    cb, cf = cut(rng, len(audio), rounds), cut(rng, len(fr), rounds)
    pool = np.full(len(audio) + 200, 0xA5, np.uint8)
    rr = Rounds(emu, p, pow_table, tmpl, 1)
    upto = fpos = 0
    for r in range(rounds):
        upto += cb[r]
        pool[23:23 + upto] = np.frombuffer(audio[:upto], np.uint8)
        part = fr[fpos:fpos + cf[r]]
        fpos += cf[r]
        rr.run(pool, [23], [len(audio) + 50], [upto], [[int(f.bitrate_index) for f in part]], padding=[pad],
               ext=[int(part[-1].mode_ext) if part else 0], final=(r == rounds - 1))
    assert rr.tag(0) == tag
    enc.close()


def test_host_side_under_sanitizers():
    """the stand-alone program (its own main; AddressSanitizer and UBSan linked in): the table builder, a CRC carried over
    rounds, the end padding, a frame made of a carry and the gain patch on it"""
    helpers.locked_make(["tag_inc_host_check"], INC_DIR)
    r = subprocess.run([os.path.join(INC_DIR, "tag_inc_host_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
    assert "FAILED" not in r.stdout


def test_symbols_are_declared_and_exported():
    lib = lamehip.load_library()
    txt = open(os.path.join(helpers.ROOT, "include", "lamehip.h")).read()
    for name in ("lamehip_batch_set_incremental_tagging", "lamehip_batch_tag_size", "lamehip_batch_tag_ptr",
                 "lamehip_batch_get_tags_all", "lamehip_batch_last_tag_ms"):
        assert name + "(" in txt and hasattr(lib, name), name
    for name in ("lh_launch_tag_resume", "lh_tag_pow_table"):
        assert hasattr(lib, name), name
    for name in ("set_incremental_tagging", "tag_size", "tag", "tags_all", "tag_ms"):
        assert hasattr(lamehip.Batch, name), name
    assert "no tagged output" not in txt
