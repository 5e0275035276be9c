"""CPU: the front masking kernels (csrc/lh_psy_finish.hip: lh_ath_scan_kernel, lh_psy_mask_kernel) and the encode kernel
that starts from their records (LhMidPsy), as SOURCE under the fiber emulator of tests/hipemu, against the oracle frame
for frame.  The shapes of tests/test_psy_finish_device.py at one or two streams of a few frames each; every case runs in
two launches, so that the second takes the clamp's previous calls, the ATH level, the block-type state and the masking
adjustment from LhStreamState alone, and every record pool is poisoned first: whatever the encode kernel reads must have
been written by this launch's kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import lamehip
from lamehip.types import LhFrameOut, struct_diff
from test_emulator import EMU_DIR, LhMidPools, LhStreamDesc, MID_FRAME

# csrc/lh_device.h: LhMidPsy = en[2][4][64], thm[2][4][64], ath_factor, masking_lower, bt_old[2][2], pad
MID_PSY = 2 * (2 * 4 * 64 * 4) + 16


PSY_DIR = os.path.join(helpers.ROOT, "tests", "hipemu_psy")


class Emu:
    """The two emulator libraries of such a launch: tests/hipemu (analysis, sub-band and encode kernels) and
    tests/hipemu_psy (the front masking kernels); an entry point is looked up in either."""

    def __init__(self):
        helpers.locked_make([], EMU_DIR)
        helpers.locked_make([], PSY_DIR)
        self.libs = (C.CDLL(os.path.join(EMU_DIR, "libhipemu_lame.so")), C.CDLL(os.path.join(PSY_DIR, "libhipemu_psy.so")))

    def __getattr__(self, name):
        for lib in self.libs:
            try:
                return getattr(lib, name)
            except AttributeError:
                pass
        raise AttributeError(name)


@pytest.fixture(scope="module")
def emu():
    return Emu()


def front_encode(emu, cfg, tab, pool, descs, states, got, nstreams, max_frames, total_frames, front=True):
    """One launch of the split pipeline under the emulator, with (front) or without the front masking kernels."""
    buf = np.full(total_frames * MID_FRAME + 64, 0x5a, dtype=np.uint8)
    psy = np.full(total_frames * MID_PSY + 64, 0x5a, dtype=np.uint8)
    pools = LhMidPools(buf.ctypes.data)
    pcm = pool.ctypes.data_as(C.c_void_p)
    emu.lh_emu_analysis(C.byref(cfg), C.byref(tab), pcm, None, descs, states, C.byref(pools), nstreams, max_frames)
    if front:
        emu.lh_emu_psy_finish(C.byref(cfg), C.byref(tab), descs, states, C.byref(pools), C.c_void_p(psy.ctypes.data), nstreams, max_frames)
    emu.lh_emu_subband(C.byref(cfg), C.byref(tab), pcm, None, descs, states, C.byref(pools), nstreams, max_frames)
    if front:
        emu.lh_emu_encode_psy_q(C.byref(cfg), C.byref(tab), pcm, None, descs, states, got, None, nstreams, C.byref(pools),
                                C.c_void_p(psy.ctypes.data))
    else:
        emu.lh_emu_encode_q(C.byref(cfg), C.byref(tab), pcm, None, descs, states, got, None, nstreams, C.byref(pools))
    return psy


def silence_then_burst(n, sr, seed=5):
    """Digital silence, then a loud burst: the ATH factor falls to its floor and snaps back; the clamp meets partitions
    whose previous calls left nothing (lim1 <= 0)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros((2, n))
    a = (2 * n) // 3
    x[:, a:] = 20000 * rng.standard_normal((2, n - a)) * np.exp(-np.arange(n - a) / 2500.0)
    return x.clip(-32768, 32767).astype(np.int16)


def _pcm(what, n, sr, seed):
    if what == "silence":
        return silence_then_burst(n, sr, seed)
    return helpers.synth_stream(seed, n, sr, burst_interval=1.0 / what)


# (settings, signal: bursts per second or "silence", frames per stream, where the second launch starts)
CASES = [
    ("cbr128_js_b3", dict(brate=128), 3, (9, 7), 4),
    ("cbr128_js_b40", dict(brate=128), 40, (10, 10), 5),
    ("cbr128_stereo", dict(brate=128, mode=0), 40, (8,), 3),
    ("cbr128_mono", dict(brate=128, channels=1), 40, (8,), 3),
    ("abr128_js", dict(abr=128), 40, (8,), 5),
    ("cbr320_48k_b40", dict(samplerate=48000, brate=320), 40, (8,), 3),
    ("cbr128_silence_burst", dict(brate=128), "silence", (12,), 7),
    ("cbr128_two_frames", dict(brate=128), 40, (2,), 1),
]


@pytest.mark.parametrize("name,kw,signal,lens,cut", CASES, ids=[c[0] for c in CASES])
def test_front_masking_kernels_source_matches_oracle(name, kw, signal, lens, cut, emu, oracle):
    kw = dict(kw)
    sr = kw.get("samplerate", 44100)
    enc = lamehip.Encoder(require_device=False, **kw)
    cfg, tab = enc.config(), enc.tables()
    assert cfg.vbr in (0, 3) and cfg.mode_gr == 2
    ns = len(lens)
    pcms = [_pcm(signal, 1152 * nf + 1105, sr, 60 + s) for s, nf in enumerate(lens)]
    if cfg.channels == 1:
        pcms = [np.stack([p[0], p[0]]) for p in pcms]
    cap = max(p.shape[1] for p in pcms)
    pool = np.zeros((ns, 2, cap), np.int16)
    for s, p in enumerate(pcms):
        pool[s, :, :p.shape[1]] = p
    size = enc.lib.lamehip_abi_sizeof(4)
    states = C.create_string_buffer(size * ns)
    for s in range(ns):
        enc.lib.lh_state_init(C.byref(states, size * s), C.byref(cfg))
    total = sum(lens)
    got = (LhFrameOut * total)()
    first = np.cumsum([0] + list(lens))
    for a, b in ((0, cut), (cut, max(lens))):
        descs = (LhStreamDesc * ns)()
        for s, nf in enumerate(lens):
            lo, hi = min(a, nf), min(b, nf)
            descs[s] = LhStreamDesc(2 * s * cap, (2 * s + 1) * cap, 0, pcms[s].shape[1], int(first[s]) + lo, lo, hi)
        front_encode(emu, cfg, tab, pool.reshape(-1), descs, states, got, ns, b - a, total)
    for s, nf in enumerate(lens):
        want = oracle.encode_frames(cfg, tab, pcms[s], max_frames=nf)
        for f in range(nf):
            d = struct_diff(want[f], got[int(first[s]) + f])
            assert not d, (name, s, f, d[:4])
    enc.close()


def test_front_launches_and_plain_ones_take_turns_on_one_stream(emu, oracle):
    """A launch behind the front kernels leaves LhStreamState as every other launch expects it, and finds what it needs in
    the state any other leaves: fused, front, split without the front kernels, front, fused over consecutive frame ranges
    -- and the state words after a front launch are, word for word, those of the same frames through the plain split launch."""
    sr = 44100
    enc = lamehip.Encoder(require_device=False, brate=128)
    cfg, tab = enc.config(), enc.tables()
    nframes = 12
    pcm = helpers.synth_stream(77, 1152 * nframes + 1105, sr, burst_interval=1.0 / 40)
    want = oracle.encode_frames(cfg, tab, pcm, max_frames=nframes)
    n = pcm.shape[1]
    pool = np.concatenate([pcm[0], pcm[1]]).astype(np.int16)
    size = enc.lib.lamehip_abi_sizeof(4)
    for plan in (("fused", "front", "split", "front", "fused"), ("split",) * 5):
        state = C.create_string_buffer(size)
        enc.lib.lh_state_init(state, C.byref(cfg))
        got = (LhFrameOut * nframes)()
        for k, how in enumerate(plan):
            a, b = (0, 2, 5, 7, 10, 12)[k], (0, 2, 5, 7, 10, 12)[k + 1]
            desc = LhStreamDesc(0, n, 0, n, a, a, b)
            if how == "fused":
                emu.lh_emu_encode(C.byref(cfg), C.byref(tab), pool.ctypes.data_as(C.c_void_p), C.byref(desc), state, got, 1)
            else:
                front_encode(emu, cfg, tab, pool, C.byref(desc), state, got, 1, b - a, nframes, front=(how == "front"))
            if k == 3:
                if how == "front":
                    after_front = state.raw
                else:
                    assert state.raw == after_front, "LhStreamState after a front launch differs from the plain split launch's"
        for f in range(nframes):
            d = struct_diff(want[f], got[f])
            assert not d, (plan, f, d[:4])
    enc.close()


def test_records_are_what_the_encode_kernel_would_have_computed(emu):
    """The scan's words per frame: the ATH factor never leaves (0, 1], falls by the reference's rule in silence and is back at 1 behind the burst;
    blocktype_old only holds the three values the state machine gives it; the padding words of every band row are zero."""
    sr = 44100
    enc = lamehip.Encoder(require_device=False, brate=128)
    cfg, tab = enc.config(), enc.tables()
    nframes = 12
    pcm = silence_then_burst(1152 * nframes + 1105, sr)
    n = pcm.shape[1]
    pool = np.concatenate([pcm[0], pcm[1]]).astype(np.int16)
    state = C.create_string_buffer(enc.lib.lamehip_abi_sizeof(4))
    enc.lib.lh_state_init(state, C.byref(cfg))
    got = (LhFrameOut * nframes)()
    desc = LhStreamDesc(0, n, 0, n, 0, 0, nframes)
    psy = front_encode(emu, cfg, tab, pool, C.byref(desc), state, got, 1, nframes, nframes)
    rec = psy[:nframes * MID_PSY].reshape(nframes, MID_PSY)
    bands = rec[:, :4096].copy().view(np.float32).reshape(nframes, 2, 2, 4, 64)      # [frame][en | thm][gr][chn][band]
    head = rec[:, 4096:].copy()
    factor = head[:, 0:4].copy().view(np.float32)[:, 0]
    mlow = head[:, 4:8].copy().view(np.float32)[:, 0]
    bt = head[:, 8:12].view(np.int8)
    assert np.all(bands[..., 61:] == 0.0)
    assert np.all(np.isfinite(bands)) and np.all(bands >= 0.0)
    assert np.all(factor > 0.0) and np.all(factor <= 1.0)
    quiet = np.float64(np.float32(0.000625))            # reference encoder.c:104-118 at loudness 0
    for f in range(1, 8):                               # frames of digital silence: eased towards `quiet' by 7.5 % a frame
        assert factor[f] == np.float32(np.float64(factor[f - 1]) * (quiet * 0.075 + 0.925)), (f, factor)
    assert factor[-1] == 1.0, "two loud frames snap it back"
    assert set(np.unique(bt).tolist()) <= {0, 2, 3}     # NORM, SHORT, STOP
    assert set(np.unique(mlow).tolist()) <= {float(np.float32(cfg.masking_lower_long)), float(np.float32(cfg.masking_lower_short))}
    enc.close()
