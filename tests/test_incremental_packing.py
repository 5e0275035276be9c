"""The drain of an incremental batch that packs on the device, without a device: the SOURCE of the drain kernels
(csrc/lh_drain.hip) run by the fiber emulator of tests/hipemu -- the scan and the gather against numpy, and the position up
to which a stream's slice is final against the host packer (csrc/lh_bitstream.c), which hands out what the reference's
lame_encode_buffer returns: the encode kernel's source with its bit packer runs one frame per launch, the drain behind every
launch -- and the host's half (csrc/lh_drain.h) as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import lamehip
from lamehip.types import LhFrameOut
from test_emulator import LhStreamDesc

DRAIN_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_drain")
EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu")
PIECE, TILE = 16, 256 * 16 * 2      # LH_DR_PIECE, LH_DR_TILE (csrc/lh_drain.h)


class LhDrainParams(C.Structure):
    _fields_ = [("sideinfo_len", C.c_int), ("frame_factor", C.c_int), ("samplerate", C.c_int), ("final", C.c_int),
                ("kbps", C.c_int16 * 16)]


class LhDrainRow(C.Structure):
    _fields_ = [("off", C.c_longlong), ("n", C.c_longlong), ("upto", C.c_longlong), ("next", C.c_longlong), ("status", C.c_int),
                ("pad", C.c_int)]


class LhDrainTile(C.Structure):
    _fields_ = [("stream", C.c_int), ("tile", C.c_int)]


# LhStreamState (csrc/lh_device.h): ... pefirbuf[19], sixteen ints (slot_lag ... status, pad[3]), then em_next_header and
# em_cursor.  (tests/test_emulator.py reads frame_number / primed / status at the same offsets.)
OFF_PEFIR = 4 * (4 * 4 * 64 + 2 + 4 + 36 + 4 + 2 + 2 + 2 * 576)
OFF_STATUS = OFF_PEFIR + 4 * (19 + 12)
OFF_NEXT = (OFF_PEFIR + 4 * (19 + 16) + 7) // 8 * 8
OFF_CURSOR = OFF_NEXT + 8


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_drain.so"], DRAIN_DIR)
    e = C.CDLL(os.path.join(DRAIN_DIR, "libhipemu_drain.so"))
    e.lh_emu_drain.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    e.lh_emu_drain_tiles.restype = C.c_longlong
    e.lh_emu_drain_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    e.lh_emu_drain_bound.restype = C.c_longlong
    e.lh_emu_drain_bound.argtypes = [C.c_longlong] * 5
    return e


@pytest.fixture(scope="module")
def emu_encode():
    helpers.locked_make([], EMU_DIR)
    return C.CDLL(os.path.join(EMU_DIR, "libhipemu_lame.so"))


def aligned(nbytes, fill=None):
    """a uint8 array on a 16-byte boundary"""
    raw = np.empty(nbytes + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    a = raw[at:at + nbytes]
    if fill is not None:
        a[:] = fill
    assert a.ctypes.data % 16 == 0
    return a


def tiles_of(emu, bounds):
    """the host's tile table and the round buffer's size for these bounds (csrc/lh_drain.h as the twin compiled it)"""
    b = np.ascontiguousarray(bounds, dtype=np.int64)
    padded = C.c_longlong(-1)
    n = emu.lh_emu_drain_tiles(b.ctypes.data, len(b), None, 0, C.byref(padded))
    tiles = (LhDrainTile * max(n, 1))()
    assert emu.lh_emu_drain_tiles(b.ctypes.data, len(b), tiles, n, None) == n
    return tiles, n, padded.value


def drain_params(cfg, lib, final):
    p = LhDrainParams(cfg.sideinfo_len, (cfg.version + 1) * 72000, cfg.samplerate, final)
    for i in range(1, 15):
        p.kbps[i] = lib.lh_tag_kbps(cfg.version, i)
    return p


@pytest.mark.parametrize("B", [1, 3, 70, 300])
def test_gather_and_scan_match_numpy(B, emu):
    """Random (drained, P) per stream in a pool of random bytes: the table is numpy's cumulative sum of the counts, each
    rounded up to 16; every gathered range equals its source; every other byte of the poisoned round buffer is untouched.
    The counts include 0, 1, under a piece, a piece, a tile less one, exact, plus one and several tiles; the source offsets
    cover all 16 residues; 70 streams cross a wave in the scan, 300 a workgroup's tile; one stream carries a status and
    gives nothing; the host's bounds are larger than the counts, so tiles behind a stream's count exist."""
    rng = np.random.default_rng(4200 + B)
    sizeof_state = emu.lh_emu_drain_sizeof_state()
    special = [0, 1, 5, 15, 16, 17, 31, 32, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 7, 3 * TILE]
    counts = [special[s % len(special)] if (B <= 3 or s % 2 == 0) else int(rng.integers(0, 3000)) for s in range(B)]
    if B == 1:
        counts = [2 * TILE + 7]
    if B == 3:
        counts = [TILE + 1, 0, 9]
    descs = (LhStreamDesc * B)()
    states = np.zeros((B, sizeof_state), np.uint8)
    drained = np.zeros(B, np.int64)
    carry = np.zeros(B, np.int64)
    bounds = np.zeros(B, np.int64)
    at = 0
    for s in range(B):
        drained[s] = int(rng.integers(0, 500))
        base = at + int(rng.integers(0, 16))
        base += (s - (base + int(drained[s]))) % 16     # the source of stream s: s % 16 bytes behind a boundary
        upto = int(drained[s]) + counts[s]
        cap = upto + int(rng.integers(0, 40))
        descs[s] = LhStreamDesc(0, 0, 0, 0, 0, 0, 0, base, cap, 1, 0)
        states[s, OFF_NEXT:OFF_NEXT + 8] = np.frombuffer(np.int64(upto).tobytes(), np.uint8)
        states[s, OFF_CURSOR:OFF_CURSOR + 8] = np.frombuffer(np.int64(max(upto - 3, 0)).tobytes(), np.uint8)
        bounds[s] = counts[s] + int(rng.integers(0, 2 * TILE))
        at = base + cap + int(rng.integers(0, 64))
    bad = B // 2 if B > 3 else -1
    if bad >= 0:
        states[bad, OFF_STATUS:OFF_STATUS + 4] = np.frombuffer(np.int32(8).tobytes(), np.uint8)
        counts[bad] = 0
    pool = aligned(at + 64)
    pool[:] = rng.integers(1, 256, len(pool), dtype=np.uint8)
    for s in range(B):
        assert (pool.ctypes.data + descs[s].bytes_base + int(drained[s])) % 16 == s % 16
    tiles, ntiles, padded = tiles_of(emu, bounds)
    guard = 256
    buf = aligned(guard + padded + guard, 0xA5)
    rows = (LhDrainRow * (B + 1))()
    p = LhDrainParams(32, 144000, 44100, 1)
    assert emu.lh_emu_drain(C.byref(p), descs, states.ctypes.data, drained.ctypes.data, carry.ctypes.data, pool.ctypes.data, rows, B,
                            tiles, ntiles, buf.ctypes.data + guard, padded) == 0
    want = np.full(len(buf), 0xA5, np.uint8)
    off = 0
    for s in range(B):
        assert (rows[s].off, rows[s].n, rows[s].status) == (off, counts[s], 8 if s == bad else 0), s
        src = descs[s].bytes_base + int(drained[s])
        want[guard + off:guard + off + counts[s]] = pool[src:src + counts[s]]
        off += (counts[s] + PIECE - 1) // PIECE * PIECE
    assert rows[B].off == off <= padded
    assert np.array_equal(buf, want)
    assert not carry.any()      # (behind the flush no header is walked)


def test_a_stream_beyond_the_round_buffer_is_left_out(emu):
    """A count the host's bound does not cover: the table says so (the host refuses the round on it), nothing is written
    outside the round buffer."""
    sizeof_state = emu.lh_emu_drain_sizeof_state()
    descs = (LhStreamDesc * 2)()
    states = np.zeros((2, sizeof_state), np.uint8)
    for s in range(2):
        descs[s] = LhStreamDesc(0, 0, 0, 0, 0, 0, 0, s * 4096, 4096, 1, 0)
        states[s, OFF_NEXT:OFF_NEXT + 8] = np.frombuffer(np.int64(1000).tobytes(), np.uint8)
    pool = aligned(8192, 7)
    drained = np.zeros(2, np.int64)
    carry = np.zeros(2, np.int64)
    tiles, ntiles, padded = tiles_of(emu, [1000, 100])      # (stream 1's bound is too small)
    buf = aligned(padded + 4096, 0xA5)
    rows = (LhDrainRow * 3)()
    p = LhDrainParams(32, 144000, 44100, 1)
    assert emu.lh_emu_drain(C.byref(p), descs, states.ctypes.data, drained.ctypes.data, carry.ctypes.data, pool.ctypes.data, rows, 2,
                            tiles, ntiles, buf.ctypes.data, padded) == 0
    assert rows[1].n == 1000 and rows[2].off > padded
    assert (buf[:1000] == 7).all() and (buf[1000:] == 0xA5).all()


def parse_frames(mp3, cfg):
    """(start, length, main_data_begin) of every frame of an MPEG audio byte string made with these settings"""
    lsf = cfg.version != 1
    rates = ([0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160] if lsf
             else [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320])
    out, at = [], 0
    while at + 4 <= len(mp3):
        assert mp3[at] == 0xFF and (mp3[at + 1] & 0xE0) == 0xE0, at
        length = (cfg.version + 1) * 72000 * rates[mp3[at + 2] >> 4] // cfg.samplerate + ((mp3[at + 2] >> 1) & 1)
        crc = 0 if (mp3[at + 1] & 1) else 2
        mdb = mp3[at + 4 + crc] if lsf else (mp3[at + 4 + crc] << 1) | (mp3[at + 5 + crc] >> 7)
        out.append((at, length, mdb))
        at += length
    assert at == len(mp3)
    return out


def landing_frames(frames, sl, pre=None):
    """Frame N lands -- its main data ends exactly on the start of a header that is already queued, its own or an earlier
    one -- when frame N + 1's back pointer equals the main-data room of frames j .. N for some j <= N.  The headers alone
    show the frames behind which the next one starts with its own data; pre[n] -- the bytes of stuffing frame n's record
    says it put in front of its data, which its back pointer leaves out -- shows the others as well."""
    landing = {}
    for n in range(len(frames) - 1):
        room, back = 0, frames[n + 1][2] + (pre[n + 1] if pre else 0)
        for j in range(n, -1, -1):
            room += frames[j][1] - sl
            if room == back:
                landing[n] = frames[j][0]
            if room >= back:
                break
    return landing


# fixture, (landing frames the test insists on: at least this many, this one among them)
POSITION_CASES = [("abr112_js_44k_silence", (6, 0)), ("cbr64_js_22k_lsf", (1, 29)), ("cbr128_js_44k", (0, None)),
                  ("vbr2_js_44k", (0, None)), ("cbr16_js_8k_lsf", (0, None))]


@pytest.mark.parametrize("name,insist", POSITION_CASES)
def test_position_rule_matches_the_host_packer(name, insist, emu, emu_encode):
    """One frame per launch through the encode kernel's source with the device packer, the state carried; behind every
    launch the emulated drain, behind the last one -- which flushes -- the drain of lamehip_batch_finish.  Every round's count
    and bytes are those lh_bs_format_frame + lh_bs_copy (lh_bs_flush at the end) make of the same records, and all of them
    together are the fixture's mp3.  The frames whose main data ends on a queued header are computed from the fixture's own
    headers (those behind which the next frame starts with stuffing: from the records as well): on exactly those the drain
    stops at the header's start instead of the packer's cursor."""
    g, pcm = helpers.load_golden(name)
    enc = lamehip.Encoder(require_device=False, **helpers.golden_encoder_kwargs(g))
    cfg, tab, lib = enc.config(), enc.tables(), enc.lib
    lib.lh_bs_flush.restype = None
    nframes = int(g["nframes"])
    want = g["mp3"].tobytes()
    frames = parse_frames(want, cfg)
    assert len(frames) == nframes
    landing = landing_frames(frames, cfg.sideinfo_len)
    assert len(landing) >= insist[0] and (insist[1] is None or insist[1] in landing), sorted(landing)
    n = pcm.shape[1]
    pcm_pool = np.concatenate([pcm[0], pcm[1]]).astype(np.int16)
    cap = nframes * 1500
    state = C.create_string_buffer(lib.lamehip_abi_sizeof(4))
    assert len(state) == emu.lh_emu_drain_sizeof_state()
    lib.lh_state_init(state, C.byref(cfg))
    got = (LhFrameOut * nframes)()
    out = aligned(cap + 64, 0)
    bs = C.create_string_buffer(64 * 1024)
    assert lib.lh_bs_init(bs) == 0
    tmp = C.create_string_buffer(65536)
    drained = np.zeros(1, np.int64)
    carry = np.zeros(1, np.int64)
    rows = (LhDrainRow * 2)()
    frame_max = max(f[1] for f in frames)
    stream, took_header, took_cursor, known = b"", {}, set(), 0
    for f in range(nframes):
        last = f == nframes - 1
        desc = LhStreamDesc(0, n, 0, n, f, f, f + 1, 0, cap, 1 if last else 0, 0)
        emu_encode.lh_emu_encode_bytes(C.byref(cfg), C.byref(tab), pcm_pool.ctypes.data_as(C.c_void_p), C.byref(desc), state, got,
                                       out.ctypes.data_as(C.c_void_p), 1)
        # the host packer on the same record
        assert lib.lh_bs_format_frame(bs, C.byref(cfg), C.byref(tab), C.byref(got[f])) == 0
        k = lib.lh_bs_copy(bs, tmp, len(tmp))
        host = tmp.raw[:k]
        if last:
            lib.lh_bs_flush(bs, C.byref(cfg), C.byref(got[f]))
            k = lib.lh_bs_copy(bs, tmp, len(tmp))
            host += tmp.raw[:k]
        # the drain, sized by the host as the library does
        bound = emu.lh_emu_drain_bound(known, 1, frame_max, cap, int(drained[0]))
        tiles, ntiles, padded = tiles_of(emu, [bound])
        buf = aligned(padded + 32, 0xA5)
        p = drain_params(cfg, lib, 1 if last else 0)
        assert emu.lh_emu_drain(C.byref(p), C.byref(desc), state, drained.ctypes.data, carry.ctypes.data, out.ctypes.data, rows, 1,
                                tiles, ntiles, buf.ctypes.data, padded) == 0
        assert rows[0].status == 0 and rows[0].off == 0
        cursor = int(np.frombuffer(state.raw[OFF_CURSOR:OFF_CURSOR + 8], np.int64)[0])
        assert rows[0].n == len(host), (f, rows[0].n, len(host), rows[0].upto, cursor)
        assert buf[:len(host)].tobytes() == host, f
        assert (buf[len(host):] == 0xA5).all()
        if not last:
            if f in landing:
                assert rows[0].upto == landing[f], f
            if rows[0].upto == cursor:
                took_cursor.add(f)
            else:
                assert rows[0].upto == cursor - cfg.sideinfo_len, f
                took_header[f] = rows[0].upto
        drained[0] += rows[0].n
        known = rows[0].next
        assert known == frames[f][0] + frames[f][1]
        stream += host
    assert stream == want
    assert took_header == landing_frames(frames, cfg.sideinfo_len, [fr.resvDrain_pre // 8 for fr in got]) and took_cursor
    assert set(landing) <= set(took_header)
    lib.lh_bs_free(bs)
    enc.close()


def test_host_side_under_sanitizers():
    """csrc/lh_drain.h (the bound, the tile table) over its cases in a stand-alone program under ASan and UBSan"""
    helpers.locked_make(["drain_host_check"], DRAIN_DIR)
    r = subprocess.run([os.path.join(DRAIN_DIR, "drain_host_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
