"""Typed input of a batch (lamehip_batch_set_sample_type): ctypes bindings of the host evaluation (csrc/lh_pcm_in.c), the
records of csrc/lh_pcm_in.h, and the test signals, for test_pcm_input.py, test_pcm_input_device.py and its child."""
import ctypes as C

import numpy as np

import helpers
import lamehip
from lamehip import PCM_DTYPES, PCM_F32, PCM_F32_UNIT, PCM_S16, PCM_S32

TYPE_NAMES = {PCM_S16: "s16", PCM_S32: "s32", PCM_F32: "f32", PCM_F32_UNIT: "f32unit"}
# kind of oracle/ref_harness.c's refh_encode_typed per (sample type, interleaved)
REF_KIND = {(PCM_F32, False): 1, (PCM_F32_UNIT, False): 2, (PCM_F32_UNIT, True): 3, (PCM_S32, False): 5, (PCM_S16, True): 8}
# the handle call of this library per kind (what the bytes are compared with where the compiled reference is absent)
HANDLE_CALL = {1: "lame_encode_buffer_float", 2: "lame_encode_buffer_ieee_float", 3: "lame_encode_buffer_interleaved_ieee_float",
               5: "lame_encode_buffer_int", 8: "lame_encode_buffer_interleaved"}


class LhInStream(C.Structure):
    _fields_ = [("n", C.c_longlong), ("stream", C.c_int), ("pad_", C.c_int)]


class LhInParams(C.Structure):
    _fields_ = [("m", C.c_float * 4), ("channels", C.c_int), ("one_plane", C.c_int), ("cap", C.c_longlong)]


def library():
    lib = lamehip.load_library()
    lib.lh_pcm_matrix_host.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]
    lib.lh_pcm_matrix_host.restype = None
    lib.lh_pcm_ingest_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    lib.lh_pcm_eval_block.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    lib.lh_pcm_eval_block.restype = None
    return lib


def matrix(lib, stype, scale, mix, scale_r):
    """float32 [4]: m00, m01, m10, m11 of lame_encode_buffer_template for the sample type and the handle's scales"""
    m = np.zeros(4, np.float32)
    lib.lh_pcm_matrix_host(stype, scale, mix, scale_r, m.ctypes.data)
    return m


def host_ingest(lib, stype, m, left, right=None, interleaved=None):
    """lh_pcm_ingest_host: float32 [2, n]; right=None: one plane (the second mirrors the first)"""
    if interleaved is not None:
        x = np.ascontiguousarray(interleaved)
        n, stride, pl, pr = x.shape[0], 2, x.ctypes.data, x.ctypes.data + x.dtype.itemsize
    else:
        left = np.ascontiguousarray(left)
        right = None if right is None else np.ascontiguousarray(right)
        n, stride, pl, pr = len(left), 1, left.ctypes.data, None if right is None else right.ctypes.data
    out = np.zeros((2, n), np.float32)
    assert lib.lh_pcm_ingest_host(stype, m.ctypes.data, pl, pr, stride, n, out[0].ctypes.data, out[1].ctypes.data) == 0
    return out


def typed_signal(stype, seed, n, sr=44100):
    """a stream of the sample type with values that are no whole 16-bit steps, [2, n]: synth_stream plus
    uniform(-0.4, 0.4), as tests/test_gpu_parity.py builds its typed buffers -- scaled to +/- 1.0 for PCM_F32_UNIT and
    by 65536 for PCM_S32 (non-zero low 16 bits); PCM_S16: synth_stream itself"""
    base = helpers.synth_stream(seed, n, sr, 1.0 / 7) if n else np.zeros((2, 0), np.int16)
    if stype == PCM_S16:
        return base
    rng = np.random.Generator(np.random.PCG64(seed))
    x = base.astype(np.float64) + rng.uniform(-0.4, 0.4, (2, n))
    if stype == PCM_F32_UNIT:
        x = x / 32767.0
    if stype == PCM_S32:
        x = x * 65536.0
    return np.ascontiguousarray(x.astype(PCM_DTYPES[stype]))


def beyond_value(stype):
    """what rows hold beyond a stream's length: never to be read"""
    return {PCM_S16: 0x7fff, PCM_S32: 0x7fffffff}.get(stype, np.nan)


def same_floats(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()
