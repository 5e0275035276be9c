"""ctypes bindings of the rate converter's host side (csrc/lh_resample.c: conversion, plan, block evaluation)
for test_resample_plan.py and test_resample_device.py."""
import ctypes as C

import numpy as np

import lamehip

FS, MFN = 1152, 1904            # MPEG-1 frame size and the samples buffered before a frame is encoded
MF_START = 528


class LhResampler(C.Structure):
    _fields_ = [("rate_in", C.c_int), ("rate_out", C.c_int), ("ratio", C.c_double), ("phases", C.c_int),
                ("taps", C.c_int), ("clock", C.c_double * 2), ("history", (C.c_float * 34) * 2),
                ("bank", (C.c_float * 34) * 641)]


class LhRsBlock(C.Structure):
    _fields_ = [("in_at", C.c_longlong), ("out_at", C.c_longlong), ("start", C.c_double), ("len", C.c_int),
                ("made", C.c_int)]

    def key(self):
        return (self.in_at, self.out_at, self.start, self.len, self.made)


class LhRsCursor(C.Structure):
    _fields_ = [("clock", C.c_double), ("in_at", C.c_longlong), ("fed", C.c_longlong), ("mf_size", C.c_long),
                ("frames", C.c_int), ("nblk", C.c_int)]


class LhRsTrunk(C.Structure):
    _fields_ = [("fs", C.c_int), ("mfn", C.c_int), ("nchunks", C.c_long), ("cap_chunks", C.c_long),
                ("after", C.POINTER(LhRsCursor)), ("blk", C.POINTER(LhRsBlock)), ("cap_blk", C.c_long)]


class LhRsStream(C.Structure):
    _fields_ = [("n", C.c_longlong), ("stream", C.c_int), ("ntrunk", C.c_int), ("tail_at", C.c_int),
                ("ntail", C.c_int)]


class LhRsMatrix(C.Structure):
    _fields_ = [("m00", C.c_float), ("m01", C.c_float), ("m10", C.c_float), ("m11", C.c_float)]


class LhRsParams(C.Structure):
    _fields_ = [("ratio", C.c_double), ("m", LhRsMatrix), ("taps", C.c_int), ("phases", C.c_int),
                ("channels", C.c_int), ("one_plane", C.c_int), ("cap_in", C.c_longlong), ("cap_out", C.c_longlong)]


LH_RS_ROW = 36


def library():
    lib = lamehip.load_library()
    lib.lh_rs_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lh_rs_block.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.lh_rs_convert_stream.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                         C.c_float, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lh_rs_free.argtypes = [C.c_void_p]
    lib.lh_rs_free.restype = None
    lib.lh_rs_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]
    lib.lh_rs_eval_block.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    lib.lh_rs_eval_block.restype = None
    lib.lh_rs_trunk_init.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.lh_rs_trunk_init.restype = None
    lib.lh_rs_trunk_free.argtypes = [C.c_void_p]
    lib.lh_rs_trunk_free.restype = None
    lib.lh_rs_trunk_extend.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    lib.lh_rs_plan_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
    return lib


def resampler(lib, rate_in, rate_out):
    rs = LhResampler()
    lib.lh_rs_init(C.byref(rs), rate_in, rate_out)
    return rs


def host_convert(lib, rate_in, rate_out, channels, scale, mix, scale_r, pcm, fs=FS, mfn=MFN):
    """lh_rs_convert_stream: (float32 [2, converted length], frames, padding)"""
    rs = LhResampler()
    l = np.ascontiguousarray(pcm[0], dtype=np.int16)
    r = np.ascontiguousarray(pcm[1], dtype=np.int16)
    pl, pr = C.c_void_p(), C.c_void_p()
    n, frames, padding = C.c_long(0), C.c_int(0), C.c_int(0)
    rc = lib.lh_rs_convert_stream(C.byref(rs), rate_in, rate_out, fs, mfn, channels, scale, mix, scale_r, l.ctypes.data,
                                  r.ctypes.data, len(l), C.byref(pl), C.byref(pr), C.byref(n), C.byref(frames),
                                  C.byref(padding))
    assert rc == 0
    out = np.zeros((2, n.value), np.float32)
    if n.value:
        C.memmove(out[0].ctypes.data, pl, 4 * n.value)
        C.memmove(out[1].ctypes.data, pr, 4 * n.value)
    lib.lh_rs_free(pl)
    lib.lh_rs_free(pr)
    return out, frames.value, padding.value


def plan(lib, rs, n, fs=FS, mfn=MFN):
    """lh_rs_plan: (blocks, length of the trunk prefix, converted length, frames, padding)"""
    cap = 64
    while True:
        blocks = (LhRsBlock * cap)()
        ntrunk, frames, padding, conv = C.c_int(0), C.c_int(0), C.c_int(0), C.c_long(0)
        k = lib.lh_rs_plan(C.byref(rs), fs, mfn, n, blocks, cap, C.byref(ntrunk), C.byref(conv), C.byref(frames),
                           C.byref(padding))
        assert k >= 0
        if k <= cap:
            return list(blocks[:k]), ntrunk.value, conv.value, frames.value, padding.value
        cap = k


def evaluate(lib, rs, blocks, conv_len, channels, scale, mix, scale_r, pcm):
    """every block of a plan through lh_rs_eval_block (the shared per-sample header on the host)"""
    l = np.ascontiguousarray(pcm[0], dtype=np.int16)
    r = np.ascontiguousarray(pcm[1], dtype=np.int16)
    out = np.full((2, conv_len), np.nan, np.float32)
    for b in blocks:
        lib.lh_rs_eval_block(C.byref(rs), C.byref(b), channels, scale, mix, scale_r, l.ctypes.data, r.ctypes.data, len(l),
                             out[0].ctypes.data, out[1].ctypes.data)
    return out


def same_floats(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()
