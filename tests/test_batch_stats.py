"""A batch's statistics (lamehip_batch_set_statistics) without a device: the SOURCE of lh_stats_resume_kernel
(csrc/lh_stats.hip) run by the fiber emulator of tests/hipemu over the CPU oracle's frame records -- in one launch, in rounds,
for several streams at once --, against the parse of the reference's own bytes (tests/stats_support.py reads header and side
info of the golden `mp3') and against the host text of the counting rule (csrc/lh_stats.h); granules and channels a stream
does not have filled with garbage; synthetic records for the bins the reference never reaches; frame counts around the
workgroup's size; the host text as a stand-alone program under AddressSanitizer and UBSan; exports and what the binding
refuses before it reaches a device.  Every check is integer equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import lamehip
import stats_support as ss
from lamehip.types import LhFrameOut

EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_stats")
WORDS = 176
GUARD = 64
REC = C.sizeof(LhFrameOut)


@pytest.fixture(scope="module")
def emu():
    helpers.locked_make(["libhipemu_stats.so"], EMU_DIR)
    e = C.CDLL(os.path.join(EMU_DIR, "libhipemu_stats.so"))
    e.lh_emu_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    e.lh_emu_stats_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    e.lh_emu_stats_host.restype = None
    assert e.lh_emu_stats_sizeof(0) == WORDS * 4 and e.lh_emu_stats_sizeof(1) == REC == 4928
    return e


_CACHE = {}


def fixture(name):
    """(records uint8 [n, REC] of the CPU oracle, per-frame keys of the golden bytes, channels, granules); made once"""
    if name not in _CACHE:
        g, pcm = helpers.load_golden(name)
        enc = lamehip.Encoder(require_device=False, **helpers.golden_encoder_kwargs(g))
        cfg, tab = enc.config(), enc.tables()
        frames = helpers.Oracle().encode_frames(cfg, tab, pcm)
        rec = np.frombuffer(bytes(frames), np.uint8).reshape(len(frames), REC).copy()
        rec.setflags(write=False)
        keys, (channels, ngr) = ss.parse(g["mp3"].tobytes())
        assert (channels, ngr) == (cfg.channels, cfg.mode_gr) and len(keys) == int(g["nframes"]) == len(frames)
        ss.check_fixture_facts(name, keys, channels, ngr)
        enc.close()
        _CACHE[name] = (rec, keys, channels, ngr)
    return _CACHE[name]


class Carries:
    """B streams' records between guard words, and the kernel over them"""

    def __init__(self, emu, B, channels, ngr):
        self.emu, self.B, self.channels, self.ngr = emu, B, channels, ngr
        self.mem = np.full(GUARD + B * WORDS + GUARD, 0x5A5A5A5A, np.int32)
        self.mem[GUARD:GUARD + B * WORDS] = 0

    def carry(self, s):
        return self.mem[GUARD + s * WORDS:GUARD + (s + 1) * WORDS]

    def launch(self, records, out_index, nframes):
        records = np.ascontiguousarray(records)
        oi, nf = np.asarray(out_index, np.int64), np.asarray(nframes, np.int32)
        assert len(oi) == len(nf) == self.B and all(o >= 0 and o + max(n, 0) <= len(records) for o, n in zip(oi, nf))
        base = self.mem[GUARD:]
        assert self.emu.lh_emu_stats(records.ctypes.data, self.B, oi.ctypes.data, nf.ctypes.data, self.channels, self.ngr, base.ctypes.data) == 0
        assert (self.mem[:GUARD] == 0x5A5A5A5A).all() and (self.mem[-GUARD:] == 0x5A5A5A5A).all(), "guard words written"


def host_text(emu, records, channels, ngr):
    out = np.zeros(WORDS, np.int32)
    records = np.ascontiguousarray(records)
    emu.lh_emu_stats_host(records.ctypes.data, len(records), channels, ngr, out.ctypes.data)
    return out


def test_parser_counts_every_golden_streams_frames():
    """the parser walks all whole-stream fixtures: its frame count is the fixture's"""
    names = sorted(f[:-4] for f in os.listdir(helpers.GOLDEN_DIR) if f.endswith(".npz") and not f.startswith("stages_"))
    assert len(names) >= 46 and all(n in names for n in ss.FIXTURES)
    for name in names:
        g = np.load(os.path.join(helpers.GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        keys, (channels, ngr) = ss.parse(g["mp3"].tobytes())
        assert len(keys) == int(g["nframes"]), name
        assert channels == (int(g["channels"]) if "channels" in g.files else 2), name
        if name in ss.FIXTURES:
            ss.check_fixture_facts(name, keys, channels, ngr)


@pytest.mark.parametrize("name", list(ss.FIXTURES))
def test_oracle_records_in_one_launch(name, emu):
    rec, keys, channels, ngr = fixture(name)
    c = Carries(emu, 1, channels, ngr)
    c.launch(rec, [0], [len(rec)])
    want = ss.flat(*ss.hist(keys, channels))
    assert (c.carry(0) == want).all()
    assert (host_text(emu, rec, channels, ngr) == want).all()


@pytest.mark.parametrize("name", list(ss.FIXTURES))
def test_oracle_records_in_uneven_rounds(name, emu):
    """rounds of 0, 1 and other frame counts: after every round the carry is the histogram of the prefix"""
    rec, keys, channels, ngr = fixture(name)
    c = Carries(emu, 1, channels, ngr)
    done = 0
    for n in [0, 1, 0, 3, 1, 7, 2, 0, 11, 5, 1000]:
        n = min(n, len(rec) - done)
        c.launch(rec[done:done + max(n, 1)], [0], [n])      # (the round's records start at the pool's first slot)
        done += n
        assert (c.carry(0) == ss.flat(*ss.hist(keys[:done], channels))).all(), "after %d frames" % done
    assert done == len(rec)
    assert (c.carry(0) == host_text(emu, rec, channels, ngr)).all()


@pytest.mark.parametrize("name", list(ss.FIXTURES))
def test_several_streams_with_ranges_of_their_own(name, emu):
    """five streams in one launch, each a different run of the pool's records, one of them none: its carry -- whatever it
    holds -- and the guard words around the array stay as they are"""
    rec, keys, channels, ngr = fixture(name)
    n = len(rec)
    ranges = [(0, n), (3, 1), (n // 2, 0), (n // 3, n - n // 3), (1, n // 2)]
    c = Carries(emu, len(ranges), channels, ngr)
    c.carry(2)[:] = np.arange(WORDS) + 1000
    c.launch(rec, [r[0] for r in ranges], [r[1] for r in ranges])
    for s, (at, k) in enumerate(ranges):
        want = ss.flat(*ss.hist(keys[at:at + k], channels)) if s != 2 else np.arange(WORDS) + 1000
        assert (c.carry(s) == want).all(), s
    # a second launch moves every stream on by its own range
    c.launch(rec, [r[0] for r in ranges], [r[1] for r in ranges])
    for s, (at, k) in enumerate(ranges):
        want = 2 * ss.flat(*ss.hist(keys[at:at + k], channels)) if s != 2 else np.arange(WORDS) + 1000
        assert (c.carry(s) == want).all(), s
    # negative frame counts are empty ranges too
    c.launch(rec, [0] * len(ranges), [-1] * len(ranges))
    assert (c.carry(0) == 2 * ss.flat(*ss.hist(keys, channels))).all()


@pytest.mark.parametrize("name", ["abr56_js_22k_lsf", "cbr16_js_8k_lsf", "mono_vbr2_44k"])
def test_granules_the_stream_does_not_have_are_not_read(name, emu):
    rec, keys, channels, ngr = fixture(name)
    dirty = rec.copy()
    gsz = REC // 4 - 8                                      # sizeof(LhGranule): four of them, then 32 bytes of tail
    assert gsz == 1224
    for gr in range(2):
        for ch in range(2):
            if gr >= ngr or ch >= channels:
                dirty[:, (2 * gr + ch) * gsz:(2 * gr + ch + 1) * gsz] = 0xA5
    assert (dirty != rec).any()
    c = Carries(emu, 1, channels, ngr)
    c.launch(dirty, [0], [len(dirty)])
    assert (c.carry(0) == ss.flat(*ss.hist(keys, channels))).all()
    assert (host_text(emu, dirty, channels, ngr) == c.carry(0)).all()


def synthetic(n, seed):
    """n records: every bit rate index 1 .. 14, every mode extension, every block type, some granules mixed"""
    rng = np.random.default_rng(seed)
    fr = (LhFrameOut * n)()
    keys = []
    for f in range(n):
        bi, me = 1 + (f + seed) % 14, int(rng.integers(0, 4))
        fr[f].bitrate_index, fr[f].mode_ext = bi, me
        bts = []
        for gr in range(2):
            for ch in range(2):
                bt, mixed = int(rng.integers(0, 4)), int(rng.integers(0, 3) == 0)
                fr[f].gr[gr][ch].block_type, fr[f].gr[gr][ch].mixed_block_flag = bt, mixed
                bts.append(4 if mixed else bt)
        keys.append((bi, me, tuple(bts)))
    return np.frombuffer(bytes(fr), np.uint8).reshape(n, REC).copy(), keys


def cut(keys, channels, ngr):
    """the keys of a stream with fewer channels or granules than the records hold"""
    return [(bi, me, tuple(bts[2 * gr + ch] for gr in range(ngr) for ch in range(channels))) for bi, me, bts in keys]


@pytest.mark.parametrize("channels,ngr", [(2, 2), (1, 2), (2, 1), (1, 1)])
def test_synthetic_records_reach_every_bin(channels, ngr, emu):
    rec, keys = synthetic(97, 5)
    want_mode, want_block = ss.hist(cut(keys, channels, ngr), channels)
    assert all(want_mode[i][4] > 0 for i in range(1, 15)) and want_block[15][4] > 0 and all(want_block[15][:4] > 0)
    assert channels == 1 or all(want_mode[15][:4] > 0)
    c = Carries(emu, 1, channels, ngr)
    c.launch(rec, [0], [len(rec)])
    assert (c.carry(0) == ss.flat(want_mode, want_block)).all()
    assert (host_text(emu, rec, channels, ngr) == c.carry(0)).all()


def test_frame_counts_around_the_workgroups_size(emu):
    nt = emu.lh_emu_stats_nt()
    assert nt == ss.NT and nt % 64 == 0
    counts = [nt - 1, nt, nt + 1, 2 * nt + 1]
    rec, keys = synthetic(sum(counts), 11)
    at = np.concatenate([[0], np.cumsum(counts)[:-1]])
    c = Carries(emu, len(counts), 2, 2)
    c.launch(rec, at, counts)
    for s, (a, k) in enumerate(zip(at, counts)):
        assert (c.carry(s) == ss.flat(*ss.hist(keys[a:a + k], 2))).all(), k
        assert c.carry(s)[15 * 5 + 4] == k


def test_host_text_under_sanitizers():
    """tests/hipemu_stats/stats_host_check.c: a program of its own, AddressSanitizer and UBSan"""
    helpers.locked_make(["stats_host_check"], EMU_DIR)
    r = subprocess.run([os.path.join(EMU_DIR, "stats_host_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "FAILED" not in r.stdout and r.stdout.count(" ok ") == 13


GETTERS = ["lamehip_batch_get_statistics", "lamehip_batch_get_statistics_all", "lamehip_batch_bitrate_hist",
           "lamehip_batch_stereo_mode_hist", "lamehip_batch_bitrate_stereo_mode_hist", "lamehip_batch_block_type_hist",
           "lamehip_batch_bitrate_block_type_hist", "lamehip_batch_bitrate_kbps"]


def test_exports_and_what_is_refused_without_a_batch():
    lib = lamehip.load_library()
    for name in GETTERS + ["lamehip_batch_set_statistics", "lamehip_batch_last_stats_ms", "lh_launch_stats"]:
        assert hasattr(lib, name), name
    buf = (C.c_int * WORDS)()
    lib.lamehip_batch_set_statistics.argtypes = [C.c_void_p, C.c_int]
    assert lib.lamehip_batch_set_statistics(None, 1) == -1
    lib.lamehip_batch_last_stats_ms.restype = C.c_float
    lib.lamehip_batch_last_stats_ms.argtypes = [C.c_void_p]
    assert lib.lamehip_batch_last_stats_ms(None) == 0.0
    for name in GETTERS:
        f = getattr(lib, name)
        if name in ("lamehip_batch_get_statistics_all", "lamehip_batch_bitrate_kbps"):
            f.argtypes = [C.c_void_p, C.c_void_p]
            assert f(None, buf) == -1, name
        elif name == "lamehip_batch_get_statistics":
            f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            assert f(None, 0, buf, buf) == -1, name
        else:
            f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            assert f(None, 0, buf) == -1, name
    assert all(v == 0 for v in buf)
    for name in ("set_statistics", "statistics", "statistics_all", "bitrate_hist", "stereo_mode_hist", "block_type_hist", "bitrate_kbps",
                 "average_kbps", "stats_ms"):
        assert callable(getattr(lamehip.Batch, name)), name


def test_the_handle_and_the_header_name_the_shared_text():
    """one text for the rule: the handle API's loop is gone, header and kernel are listed where the library is made"""
    csrc = os.path.join(helpers.PKG, "csrc")
    api = open(os.path.join(csrc, "lh_api.cpp")).read()
    assert "lh_stats_count_frame(&g->hist" in api and "gr < 2; gr++)\n                for (int ch = 0; ch < g->cfg.channels" not in api
    mk = open(os.path.join(csrc, "Makefile")).read()
    for var in ("HOST ", "DEVOBJ ", "DEVSRC "):
        line = [ln for ln in mk.replace("\\\n", " ").splitlines() if ln.startswith(var)][0]
        assert "lh_stats" in line, var
