"""Incremental converting batches whose streams arrive at rates of their own (lamehip_batch_set_stream_in_samplerate):
what test_mixed_rates_plan.py and test_mixed_rates_device.py share -- the rates, the ragged chunks, ctypes bindings of the
pass-through plan and the class record (csrc/lh_resample.c, csrc/lh_rs_sample.h), and the host chain of a stream at any of
the rates: lh_rs_block driven call by call where the reference converts, fill_buffer's copy restated where it does not."""
import ctypes as C

import numpy as np

import append_resample_support as asup
import resample_support as rsup
from resample_support import FS, MFN, MF_START

OUT = 44100
# every stream of the pool at its own rate, all to 44.1 kHz: 147 phases / 31 taps; 441 phases capped to 320, upwards;
# 2 phases; an integer ratio (32 taps, 1 phase); blocks of several tiles; 5.5 outputs per input; just outside the window
# the reference passes through; and two rates inside it
RATES = [48000, 32000, 22050, 88200, 96000, 8000, 44130, 44100, 44110]
CHUNKS = [0, 1, 1151, 1152, 1153, 4000]
CLASSES_MAX = 16


class LhRsClass(C.Structure):
    _fields_ = [("ratio", C.c_double), ("taps", C.c_int), ("phases", C.c_int), ("identity", C.c_int),
                ("bank_at", C.c_longlong)]


BANK_FLOATS = 641 * rsup.LH_RS_ROW         # floats a class's bank takes in the one allocation


def library():
    lib = asup.library()
    lib.lh_rs_needed.argtypes = [C.c_int, C.c_int]
    lib.lh_rs_init_identity.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lh_rs_init_identity.restype = None
    lib.lh_rs_is_identity.argtypes = [C.c_void_p]
    lib.lh_rs_block_tiles_class.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return lib


def converter(lib, rate_in, rate_out=OUT):
    """the converter a stream at rate_in is planned with: lh_rs_init's, or the pass-through one"""
    rs = rsup.LhResampler()
    if lib.lh_rs_needed(rate_in, rate_out):
        lib.lh_rs_init(C.byref(rs), rate_in, rate_out)
    else:
        lib.lh_rs_init_identity(C.byref(rs), rate_in, rate_out)
    return rs


def block_tiles(lib, rs, block, stream, cls):
    n = lib.lh_rs_block_tiles_class(C.byref(rs), C.byref(block), stream, cls, None, 0)
    tiles = (asup.LhRsTile * max(n, 1))()
    assert lib.lh_rs_block_tiles_class(C.byref(rs), C.byref(block), stream, cls, tiles, n) == n
    return list(tiles[:n])


class PassChain:
    """One stream the reference does not convert, the way lame_encode_buffer and lame_encode_flush drive fill_buffer
    (reference util.c:913-920, lame.c:1708-1772, 2075-2120): every call is cut into blocks of min(frame size, what is left
    of the call), made = used; the flush owes nothing for a converter's delay and feeds bunches of mf_needed - mf_size
    zeros.  The interface of append_resample_support.HostChain; x: float32 [2, n] behind the PCM matrix."""

    def __init__(self, channels=2):
        self.channels = channels
        self.fed = self.frames = self.at = 0
        self.mf = MF_START
        self.blocks = []
        self.out = [[], []]

    def call(self, x):
        m, pos, first = x.shape[1], 0, len(self.blocks)
        while m > 0:
            made = min(FS, m)
            self.blocks.append((self.at, self.fed, 0.0, m, made))
            self.out[0].append(np.array(x[0, pos:pos + made], np.float32))
            self.out[1].append(np.array(x[1, pos:pos + made], np.float32) if self.channels == 2 else np.zeros(made, np.float32))
            self.fed += made
            self.mf += made
            if self.mf >= MFN:
                self.frames += 1
                self.mf -= FS
            self.at += made
            pos += made
            m -= made
        return self.blocks[first:]

    def state(self):
        return (0.0, self.at, self.fed, self.mf, self.frames)

    def flush(self):
        first = len(self.blocks)
        owed = int(576 + self.fed - FS * self.frames)
        padding = FS - owed % FS
        if padding < 576:
            padding += FS
        left = (owed + padding) // FS
        while left > 0:
            before = self.frames
            bunch = max(1, min(1152, MFN - self.mf))
            self.call(np.zeros((2, bunch), np.float32))
            left -= 1 if self.frames != before else 0
        return self.blocks[first:], padding

    def floats(self):
        return np.stack([np.concatenate(p) if p else np.zeros(0, np.float32) for p in self.out])


def chain(lib, rate_in, channels=2, rate_out=OUT):
    """the host chain of a stream at rate_in"""
    if lib.lh_rs_needed(rate_in, rate_out):
        return asup.HostChain(lib, rate_in, rate_out, channels)
    return PassChain(channels)


def rounds_of(nstreams, extra=0):
    """the chunk every stream gets in every round: CHUNKS rotated by the stream's number, so that every round has a stream
    with an empty call and every stream meets every size; `extra' more samples in a last round"""
    rounds = [[CHUNKS[(r + s) % len(CHUNKS)] for s in range(nstreams)] for r in range(len(CHUNKS))]
    if extra:
        rounds.append([extra + 11 * s for s in range(nstreams)])
    return rounds
