"""Incremental batches that convert the rate (lamehip_batch_set_incremental_resampling): ctypes bindings of the plan that
follows the calls (csrc/lh_resample.c: lh_rs_plan_call, lh_rs_plan_flush, lh_rs_block_tiles) and the host chain the
device conversion is compared with -- lh_rs_block driven call by call, then the handle's flush loop --, for
test_append_resample_plan.py and test_append_resample_device.py."""
import ctypes as C

import numpy as np

import resample_support as rsup
from resample_support import FS, MFN, MF_START

SPAN_MAX = 1216                 # LH_RS_SPAN_MAX: input positions a tile's outputs may touch


class LhRsTile(C.Structure):
    _fields_ = [("in_at", C.c_longlong), ("out_at", C.c_longlong), ("start", C.c_double), ("k0", C.c_int),
                ("count", C.c_int), ("stream", C.c_int), ("pad_", C.c_int)]


def library():
    lib = rsup.library()
    lib.lh_rs_cursor_init.argtypes = [C.c_void_p]
    lib.lh_rs_cursor_init.restype = None
    lib.lh_rs_plan_call.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lh_rs_plan_flush.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.lh_rs_block_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return lib


def cursor(lib):
    c = rsup.LhRsCursor()
    lib.lh_rs_cursor_init(C.byref(c))
    return c


def cursor_key(c):
    return (c.clock, c.in_at, c.fed, c.mf_size, c.frames)


def plan_call(lib, rs, cur, m):
    """lh_rs_plan_call at the cursor (which advances): the call's blocks, asked for twice -- counted, then written"""
    probe = rsup.LhRsCursor.from_buffer_copy(cur)
    n = lib.lh_rs_plan_call(C.byref(rs), FS, MFN, C.byref(probe), m, None, 0)
    blocks = (rsup.LhRsBlock * max(n, 1))()
    assert lib.lh_rs_plan_call(C.byref(rs), FS, MFN, C.byref(cur), m, blocks, n) == n
    assert cursor_key(probe) == cursor_key(cur)
    return list(blocks[:n])


def plan_flush(lib, rs, cur):
    """lh_rs_plan_flush from the cursor (which advances to the stream's end): (blocks, padding)"""
    probe, pad = rsup.LhRsCursor.from_buffer_copy(cur), C.c_int(0)
    n = lib.lh_rs_plan_flush(C.byref(rs), FS, MFN, C.byref(probe), None, 0, C.byref(pad))
    blocks = (rsup.LhRsBlock * max(n, 1))()
    assert lib.lh_rs_plan_flush(C.byref(rs), FS, MFN, C.byref(cur), blocks, n, C.byref(pad)) == n
    return list(blocks[:n]), pad.value


def block_tiles(lib, rs, block, stream=0):
    n = lib.lh_rs_block_tiles(C.byref(rs), C.byref(block), stream, None, 0)
    tiles = (LhRsTile * max(n, 1))()
    assert lib.lh_rs_block_tiles(C.byref(rs), C.byref(block), stream, tiles, n) == n
    return list(tiles[:n])


class HostChain:
    """One stream through lh_rs_block the way lame_encode_buffer drives it (reference lame.c:1708-1772): every call of m
    input samples is cut into blocks of want = FS and len = what is left of the call; then the flush loop of
    lame_encode_flush, restated as tests/test_resample_plan.py restates it.  x: float32 [2, n] behind the PCM matrix;
    channels = 1: the second plane of the output is zero and its converter is never run."""

    def __init__(self, lib, rate_in, rate_out, channels=2):
        self.lib, self.channels = lib, channels
        self.rs = rsup.resampler(lib, rate_in, rate_out)
        self.fed = self.frames = self.at = 0
        self.mf = MF_START
        self.blocks = []                # (in_at, out_at, start, len, made) of every block so far
        self.out = [[], []]

    def call(self, x):
        """feeds x [2, m]; returns the blocks of this call"""
        m, pos, first = x.shape[1], 0, len(self.blocks)
        buf = np.zeros((2, FS), np.float32)
        while m > 0:
            start, used, made = self.rs.clock[0], C.c_int(0), 0
            for ch in range(self.channels):
                src = np.ascontiguousarray(x[ch, pos:pos + m], dtype=np.float32)
                made = self.lib.lh_rs_block(C.byref(self.rs), ch, buf[ch].ctypes.data, FS, src.ctypes.data, m, C.byref(used))
            self.blocks.append((self.at, self.fed, start, m, made))
            self.out[0].append(buf[0, :made].copy())
            self.out[1].append(buf[1, :made].copy() if self.channels == 2 else np.zeros(made, np.float32))
            self.fed += made
            self.mf += made
            if self.mf >= MFN:
                self.frames += 1
                self.mf -= FS
            assert used.value > 0
            self.at += used.value
            pos += used.value
            m -= used.value
        return self.blocks[first:]

    def state(self):
        return (self.rs.clock[0], self.at, self.fed, self.mf, self.frames)

    def flush(self):
        """the flush from here: (blocks, padding); the chain ends at the stream's converted length and frame count"""
        ratio, first = self.rs.ratio, len(self.blocks)
        owed = int(576 + self.fed - FS * self.frames)
        owed = int(owed + 16. / ratio)
        padding = FS - owed % FS
        if padding < 576:
            padding += FS
        left = (owed + padding) // FS
        while left > 0:
            before = self.frames
            bunch = max(1, min(1152, int((MFN - self.mf) * ratio)))
            self.call(np.zeros((2, bunch), np.float32))
            left -= 1 if self.frames != before else 0
        return self.blocks[first:], padding

    def floats(self):
        """float32 [2, converted so far]"""
        return np.stack([np.concatenate(p) if p else np.zeros(0, np.float32) for p in self.out])
