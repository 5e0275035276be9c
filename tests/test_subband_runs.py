"""The sub-band kernel (csrc/lh_subband.hip) works through a stream in runs of LH_SB_RUN frames per workgroup: the granule
before a run is recomputed from the PCM, inside a run the overlap is carried from frame to frame, and after a launch's last
frame it goes to LhStreamState.sb_prev.  These cases put every remainder of a stream's length against the run length, both
frame geometries, every input path of the kernel's staging, frame windows and launch sequences through the split pipeline
and compare every frame's payload with the oracle's, field by field."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers
import lamehip
from lamehip import PCM_F32
from lamehip.types import LhFrameOut, struct_diff

NORM, START, SHORT, STOP = 0, 1, 2, 3


def run_length():
    """LH_SB_RUN as the kernel's source has it"""
    src = open(os.path.join(helpers.PKG, "csrc", "lh_subband.hip")).read()
    return int(re.search(r"^#define LH_SB_RUN (\d+)", src, re.M).group(1))


R = run_length()
# stream k of a run-boundary batch has k + 1 frames of PCM: every remainder against the run length occurs (a longer run
# than 40 extends the range to twice the run plus one)
NSTREAMS = 40 if R <= 40 else 2 * R + 1

# name -> (sample rate, encoder settings, streams, burst interval in s, seed of stream 0; the right channel's seed for the case
# whose channels are independent signals)
BATCHES = {
    # 44.1 kHz joint stereo CBR 128, dense bursts
    "js": (44100, dict(brate=128), NSTREAMS, 1 / 20.0, 7000, None),
    # the same in dual-channel mode with unrelated channels.  In (joint) stereo the reference couples the channels' block
    # types (lame_init_params: short_block_allowed becomes short_block_coupled), so only here can a frame's two channels --
    # the workgroup's two waves -- differ in block type.
    "dual": (44100, dict(brate=128, mode=2), NSTREAMS, 1 / 20.0, 7000, 7500),
    # 22.05 kHz CBR 64: the -DLH_LSF object, one granule per frame
    "lsf": (22050, dict(brate=64), max(16, R), 1 / 33.0, 7000, None),
}
_cache = {}


def batch_case(name, orc):
    """PCM, encoder and the oracle's frames of a run-boundary batch (computed once per session and left alone)"""
    if name not in _cache:
        sr, kw, n, burst, seed, seed_r = BATCHES[name]
        fs = 1152 if sr >= 32000 else 576
        pcms = []
        for k in range(n):
            x = helpers.synth_stream(seed + k, fs * (k + 1), sr, burst)
            if seed_r is not None:
                x = np.stack([x[0], helpers.synth_stream(seed_r + k, fs * (k + 1), sr, 1 / 27.0)[1]])
            pcms.append(x)
        enc = lamehip.Encoder(sr, require_device=False, **kw)
        cfg, tab = enc.config(), enc.tables()
        want = [orc.encode_frames(cfg, tab, x) for x in pcms]
        enc.close()
        _cache[name] = (sr, kw, pcms, want)
    return _cache[name]


def block_types(cfg, want):
    """(the block types that occur, the number of granules whose two channels differ) in the oracle's frames"""
    seen, differ = set(), 0
    for frames in want:
        for f in frames:
            for g in range(cfg.mode_gr):
                a, b = f.gr[g][0].block_type, f.gr[g][1].block_type
                seen |= {a, b}
                differ += a != b
    return seen, differ


def assert_frames(want, got, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in range(len(want)):
        d = struct_diff(want[f], got[f])
        assert not d, (what, f, d[:4])


def encode_batch(enc, pcms, mono=False, sample_type=None):
    b = lamehip.Batch(enc, len(pcms), max(x.shape[1] for x in pcms) + 16)
    if sample_type is not None:
        b.set_sample_type(sample_type)
    for s, x in enumerate(pcms):
        if sample_type is not None:
            b.set_input(s, np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1]))
        elif mono:
            b.set_pcm(s, x[0])
        else:
            b.set_pcm(s, x[0], x[1])
    b.encode()
    assert b.kernel_parts_ms()[0], "the batch did not go through the split pipeline"
    return b


def check_run_boundaries(name, orc, window=None):
    sr, kw, pcms, want = batch_case(name, orc)
    enc = lamehip.Encoder(sr, **kw)
    cfg = enc.config()
    # what the comparison is worth: the lengths cover every remainder, the signal every block type
    lens = sorted(len(w) for w in want)
    assert lens == list(range(lens[0], lens[0] + len(lens))) and len(lens) >= R, lens
    seen, differ = block_types(cfg, want)
    assert seen >= {NORM, START, SHORT, STOP}, seen
    if name == "dual":
        assert differ > 0
    b = encode_batch(enc, pcms)
    if window:
        assert b.windows() > 1
    for s in range(len(pcms)):
        assert_frames(want[s], b.get_frames(s), (name, s))
    b.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["js", "dual", "lsf"])
def test_run_boundaries(name, oracle):
    """Streams of 1, 2, ... frames of PCM in one batch: runs that end anywhere in a stream, priming granules before the stream
    and inside it, all four block types (and, in dual-channel mode, frames whose two channels differ in block type)."""
    check_run_boundaries(name, oracle)


@pytest.mark.gpu
def test_run_boundaries_in_frame_windows(oracle, monkeypatch):
    """The joint-stereo batch again in windows of three frames per stream: mid_rel is not zero and a window ends inside a run."""
    monkeypatch.setenv("LAMEHIP_MID_WINDOW", "3")
    check_run_boundaries("js", oracle, window=3)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["mono", "float32"])
def test_other_inputs(how, oracle):
    """A mono stream (the second wave's plane holds zeros or the copy the batch makes) and float32 input (the staging's float
    path: the pool the ingest kernel leaves), a dozen frames each."""
    sr, nframes = 44100, 12
    x = helpers.synth_stream(7900, 1152 * nframes, sr, 1 / 20.0)
    if how == "mono":
        enc = lamehip.Encoder(sr, brate=96, channels=1)
        x = np.stack([x[0], x[0]])
        b = encode_batch(enc, [x], mono=True)
    else:
        enc = lamehip.Encoder(sr, brate=128)
        b = encode_batch(enc, [x.astype(np.float32)], sample_type=PCM_F32)
    cfg, tab = enc.config(), enc.tables()
    want = oracle.encode_frames(cfg, tab, x)
    assert SHORT in block_types(cfg, [want])[0]
    assert_frames(want, b.get_frames(0), how)
    b.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("middle", ["split", "fused"])
def test_three_launches(middle, oracle, monkeypatch):
    """One stream in three consecutive launches of an incremental batch (frame_begin > 0 in the second and third): all three
    through the split pipeline, and with the fused kernel taking the middle one -- sb_prev handed over in both directions.
    An incremental batch hands out bytes, not records: they are compared with the host packer's bytes of the oracle's frames,
    which carry every field of the payload."""
    sr = 44100
    enc = lamehip.Encoder(sr, brate=128)
    cfg, tab = enc.config(), enc.tables()
    x = helpers.synth_stream(7950, 1152 * 30 + 77, sr, 1 / 20.0)
    want = oracle.encode_frames(cfg, tab, x)
    assert SHORT in block_types(cfg, [want])[0]
    b = lamehip.Batch(enc, 1, x.shape[1] + 16)
    cuts = [0, 1152 * 9 + 5, 1152 * 20 + 900, x.shape[1]]
    got, kinds = b"", []
    for k in range(3):
        b.append(0, np.ascontiguousarray(x[0][cuts[k]:cuts[k + 1]]), np.ascontiguousarray(x[1][cuts[k]:cuts[k + 1]]))
        monkeypatch.setenv("LAMEHIP_SPLIT_DENY", "1" if (middle == "fused" and k == 1) else "0")
        if k < 2:
            assert b.encode_available() > 0
        else:
            b.finish()
        kinds.append(bool(b.kernel_parts_ms()[0]))
        got += b.drain(0)
    assert kinds == [True, middle == "split", True], kinds
    assert got == helpers.pack_frames(enc.lib, cfg, tab, want)
    b.close()
    enc.close()


def test_run_boundaries_kernel_source(oracle):
    """The run-boundary lengths 1, 2, R - 1, R, R + 1 and 2 R + 1 frames through the kernels' source under the CPU emulator
    (tests/hipemu): analysis kernels, sub-band kernel, the encode kernel of the split pipeline -- one launch, six streams."""
    from test_emulator import EMU_DIR, LhMidPools, LhStreamDesc, MID_FRAME
    helpers.locked_make([], EMU_DIR)
    emu = C.CDLL(os.path.join(EMU_DIR, "libhipemu_lame.so"))
    sr = 44100
    lens = sorted({1, 2, R - 1, R, R + 1, 2 * R + 1} - {0})
    enc = lamehip.Encoder(sr, brate=128, require_device=False)
    cfg, tab = enc.config(), enc.tables()
    pcms = [helpers.synth_stream(7000 + k, 1152 * (n + 2), sr, 1 / 20.0) for k, n in enumerate(lens)]
    want = [oracle.encode_frames(cfg, tab, x, max_frames=n) for x, n in zip(pcms, lens)]
    assert SHORT in block_types(cfg, want)[0]
    pool = np.concatenate([np.concatenate([x[0], x[1]]) for x in pcms]).astype(np.int16)
    total = sum(lens)
    descs = (LhStreamDesc * len(lens))()
    ssz = enc.lib.lamehip_abi_sizeof(4)
    states = C.create_string_buffer(ssz * len(lens))
    at, off = 0, 0
    for s, (x, n) in enumerate(zip(pcms, lens)):
        m = x.shape[1]
        descs[s] = LhStreamDesc(off, off + m, 0, m, at, 0, n)
        enc.lib.lh_state_init(C.byref(states, ssz * s), C.byref(cfg))
        at += n
        off += 2 * m
    got = (LhFrameOut * total)()
    buf = np.full(total * MID_FRAME + 64, 0x5a, dtype=np.uint8)
    pools = LhMidPools(buf.ctypes.data)
    pcm = pool.ctypes.data_as(C.c_void_p)
    emu.lh_emu_analysis(C.byref(cfg), C.byref(tab), pcm, None, descs, states, C.byref(pools), len(lens), max(lens))
    emu.lh_emu_subband(C.byref(cfg), C.byref(tab), pcm, None, descs, states, C.byref(pools), len(lens), max(lens))
    emu.lh_emu_encode_q(C.byref(cfg), C.byref(tab), pcm, None, descs, states, got, None, len(lens), C.byref(pools))
    at = 0
    for s, n in enumerate(lens):
        assert_frames(want[s], got[at:at + n], (n, s))
        at += n
    enc.close()
