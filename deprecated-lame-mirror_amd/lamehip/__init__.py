"""lamehip -- thin ctypes host binding over liblamehip.so (the C ABI in
include/lamehip.h).  It mirrors the reference's lame.h call sequence
(lame_init -> lame_set_* -> lame_init_params -> lame_encode_buffer ->
lame_encode_flush -> lame_close) and adds the batch entry points.  There is no
Python or CPU implementation of the encode path here: if the HIP library is
missing, importing the binding's loader fails loudly.
"""
import ctypes as C
import os

import numpy as np

from .types import LhConfig, LhFrameOut, LhTables  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LAMEHIP_LIB", os.path.join(_HERE, "liblamehip.so"))   # LAMEHIP_LIB: profiling build

ERR_NODEVICE = -10
STEREO, JOINT_STEREO = 0, 1
# sample types of a batch (LAMEHIP_PCM_* in include/lamehip.h) and the element each is made of
PCM_S16, PCM_S32, PCM_F32, PCM_F32_UNIT = 0, 1, 2, 3
PCM_DTYPES = {PCM_S16: np.dtype(np.int16), PCM_S32: np.dtype(np.int32), PCM_F32: np.dtype(np.float32),
              PCM_F32_UNIT: np.dtype(np.float32)}

_lib = None


def load_library():
    """Load liblamehip.so (built in-tree by __graft_entry__.build()); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "liblamehip.so not found at %s: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the encode path has no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.lame_init.restype = C.c_void_p
    for name in ("lame_set_in_samplerate", "lame_set_num_channels", "lame_set_brate", "lame_set_mode",
                 "lame_set_quality", "lame_set_VBR", "lame_set_bWriteVbrTag", "lame_set_out_samplerate"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int]
    lib.lame_init_params.argtypes = [C.c_void_p]
    lib.lame_encode_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lame_encode_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.lame_close.argtypes = [C.c_void_p]
    lib.lame_get_lametag_frame.restype = C.c_size_t
    lib.lame_get_lametag_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.lame_get_frameNum.argtypes = [C.c_void_p]
    lib.lamehip_last_error.restype = C.c_char_p
    lib.lamehip_get_config.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.lamehip_get_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.lamehip_batch_create.restype = C.c_void_p
    lib.lamehip_batch_create.argtypes = [C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_batch_create_on.restype = C.c_void_p
    lib.lamehip_batch_create_on.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_set_device.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_batch_destroy.argtypes = [C.c_void_p]
    lib.lamehip_batch_set_pcm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    lib.lamehip_batch_set_pcm_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    lib.lamehip_batch_set_length.argtypes = [C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_batch_pcm_device_ptr.restype = C.c_void_p
    lib.lamehip_batch_pcm_device_ptr.argtypes = [C.c_void_p]
    lib.lamehip_batch_encode.argtypes = [C.c_void_p]
    lib.lamehip_batch_pack_all.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    lib.lamehip_batch_sync.argtypes = [C.c_void_p]
    lib.lamehip_batch_reset.argtypes = [C.c_void_p]
    lib.lamehip_batch_frames.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_batch_pack.restype = C.c_long
    lib.lamehip_batch_pack.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    lib.lamehip_batch_get_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lamehip_batch_get_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lamehip_batch_last_kernel_ms.restype = C.c_float
    lib.lamehip_batch_last_kernel_ms.argtypes = [C.c_void_p]
    lib.lamehip_batch_last_kernel_parts_ms.restype = C.c_int
    lib.lamehip_batch_last_kernel_parts_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.lamehip_batch_kernel_waves.argtypes = [C.c_void_p]
    lib.lamehip_batch_last_windows.restype = C.c_int
    lib.lamehip_batch_last_windows.argtypes = [C.c_void_p]
    lib.lamehip_batch_set_sample_type.argtypes = [C.c_void_p, C.c_int]
    lib.lamehip_batch_set_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_batch_set_input_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_long]
    lib.lamehip_batch_input_host_ptr.restype = C.c_void_p
    lib.lamehip_batch_input_host_ptr.argtypes = [C.c_void_p]
    lib.lamehip_batch_last_ingest_ms.restype = C.c_float
    lib.lamehip_batch_last_ingest_ms.argtypes = [C.c_void_p]
    _lib = lib
    return lib


def last_error():
    return load_library().lamehip_last_error().decode()


def _is_device_array(x):
    """a torch tensor on a GPU, or anything else that says where its samples live the same way (torch is never imported)"""
    return hasattr(x, "data_ptr") and bool(getattr(x, "is_cuda", False))


def _check_input(x, dtype, what, who="set_input"):
    """x as the batch's set_input / append_input takes it -- a numpy array, or a device array, of exactly `dtype',
    C-contiguous: never cast"""
    if _is_device_array(x):
        name = str(x.dtype).split(".")[-1]
        if name != dtype.name:
            raise TypeError("%s: %s is %s, the batch's sample type takes %s" % (who, what, name, dtype.name))
        if not x.is_contiguous():
            raise ValueError("%s: %s is not contiguous" % (who, what))
        return x
    x = np.asarray(x)
    if x.dtype != dtype:
        raise TypeError("%s: %s is %s, the batch's sample type takes %s" % (who, what, x.dtype.name, dtype.name))
    return np.ascontiguousarray(x)


class Encoder:
    """One stream behind the lame.h call sequence."""

    def __init__(self, samplerate=44100, brate=128, mode=None, quality=None, require_device=True, write_tag=False,
                 vbr_q=None, out_samplerate=0, abr=None, channels=2, device=None, vbr_mode=4, error_protection=False):
        self.lib = load_library()
        self.h = C.c_void_p(self.lib.lame_init())
        if device is not None:      # HIP device of the handle's own launches (lamehip_set_device)
            self.lib.lamehip_set_device(self.h, int(device))
        self.lib.lame_set_in_samplerate(self.h, samplerate)
        if out_samplerate:
            self.lib.lame_set_out_samplerate(self.h, out_samplerate)
        self.lib.lame_set_num_channels(self.h, channels)  # 1: mono (only the left buffer is read)
        self.channels = channels
        if abr is not None:         # ABR at a mean bitrate of `abr' kb/s (the reference's --abr n)
            self.lib.lame_set_VBR(self.h, 3)
            self.lib.lame_set_VBR_mean_bitrate_kbps(self.h, abr)
        elif vbr_q is None:
            self.lib.lame_set_brate(self.h, brate)
        else:                       # VBR at quality vbr_q (the reference's -V n): 4 vbr_mtrh, 1 vbr_mt, 2 vbr_rh (--vbr-old)
            self.lib.lame_set_VBR(self.h, vbr_mode)
            self.lib.lame_set_VBR_q(self.h, vbr_q)
        self.lib.lame_set_bWriteVbrTag(self.h, 1 if write_tag else 0)
        if error_protection:        # CRC-16 behind the header (the reference's -p)
            self.lib.lame_set_error_protection(self.h, 1)
        if mode is not None:
            self.lib.lame_set_mode(self.h, mode)
        if quality is not None:
            self.lib.lame_set_quality(self.h, quality)
        self.rc = self.lib.lame_init_params(self.h)
        if self.rc == ERR_NODEVICE and not require_device:
            return
        if self.rc != 0:
            msg = last_error()
            self.close()
            raise RuntimeError("lame_init_params failed (%d): %s" % (self.rc, msg))

    def config(self):
        c = LhConfig()
        assert self.lib.lamehip_get_config(self.h, C.byref(c), C.sizeof(c)) == C.sizeof(c)
        return c

    def tables(self):
        t = LhTables()
        assert self.lib.lamehip_get_tables(self.h, C.byref(t), C.sizeof(t)) == C.sizeof(t)
        return t

    def encode(self, left, right=None):
        left = np.ascontiguousarray(left, dtype=np.int16)
        right = left if right is None else np.ascontiguousarray(right, dtype=np.int16)   # mono: not read
        n = len(left)
        buf = C.create_string_buffer(int(1.25 * n) + 7200)
        k = self.lib.lame_encode_buffer(self.h, left.ctypes.data, right.ctypes.data, n, buf, len(buf))
        if k < 0:
            raise RuntimeError("lame_encode_buffer failed (%d): %s" % (k, last_error()))
        return buf.raw[:k]

    def flush(self):
        buf = C.create_string_buffer(4 * 7200)
        k = self.lib.lame_encode_flush(self.h, buf, len(buf))
        if k < 0:
            raise RuntimeError("lame_encode_flush failed (%d): %s" % (k, last_error()))
        return buf.raw[:k]

    def lametag_frame(self):
        """Final Xing/Info + LAME tag frame (b"" when the tag is off)."""
        buf = C.create_string_buffer(2880)
        k = self.lib.lame_get_lametag_frame(self.h, buf, len(buf))
        return buf.raw[:k]

    def close(self):
        if self.h:
            self.lib.lame_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """B independent streams with common settings, encoded by one kernel launch."""

    def __init__(self, enc, nstreams, capacity, device=None):
        """device: HIP device index the batch lives on (lamehip_batch_create_on); None = the calling
        thread's current device."""
        self.lib = enc.lib
        self.enc = enc
        self.n = nstreams
        self.capacity = capacity
        if device is None:
            self.b = C.c_void_p(self.lib.lamehip_batch_create(enc.h, nstreams, capacity))
        else:
            self.b = C.c_void_p(self.lib.lamehip_batch_create_on(int(device), enc.h, nstreams, capacity))
        if not self.b:
            raise RuntimeError("lamehip_batch_create failed: %s" % last_error())
        self.sample_type = PCM_S16

    def set_sample_type(self, t):
        """The element type of the batch's input (PCM_S16 / PCM_S32 / PCM_F32 / PCM_F32_UNIT: int16, int32 at +/- 2^31,
        float32 at +/- 32768, float32 at +/- 1.0).  Before any PCM is handed over; other than PCM_S16, encode() turns the
        input pool into the floats the kernels read with a kernel of its own (ingest_ms())."""
        rc = self.lib.lamehip_batch_set_sample_type(self.b, int(t))
        if rc:
            raise RuntimeError("lamehip_batch_set_sample_type failed (%d): %s" % (rc, last_error()))
        self.sample_type = int(t)

    def set_input(self, s, left=None, right=None, interleaved=None):
        """Stream s's samples in the batch's sample type: planar `left' / `right' (right=None: mono), or one interleaved
        array [n, 2] (as `interleaved', or as a two-dimensional `left').  numpy arrays go through the pinned mirror; arrays
        that live on the batch's GPU (anything with data_ptr() and is_cuda, such as a torch tensor) are copied on the
        device -- whatever produced them must have finished.  The dtype must be the batch's: nothing is cast."""
        ptrs, stride, n, on_device, keep = self._input_args("set_input", left, right, interleaved)
        fn = self.lib.lamehip_batch_set_input_device if on_device else self.lib.lamehip_batch_set_input
        rc = fn(self.b, s, ptrs[0], ptrs[1], stride, n)
        if rc:
            raise RuntimeError("lamehip_batch_set_input failed (%d): %s" % (rc, last_error()))

    def _input_args(self, who, left, right, interleaved):
        """what set_input / append_input hand to the library: (left pointer, right pointer), stride, samples, whether the
        arrays live on the device, and the arrays themselves (to be kept alive across the call)"""
        dtype = PCM_DTYPES[self.sample_type]
        if interleaved is None and left is not None and right is None and len(getattr(left, "shape", ())) == 2:
            interleaved, left = left, None
        if interleaved is not None:
            if left is not None or right is not None:
                raise ValueError("%s: planar arrays or an interleaved one, not both" % who)
            x = _check_input(interleaved, dtype, "interleaved", who)
            if len(x.shape) != 2 or x.shape[1] != 2:
                raise ValueError("%s: an interleaved array is [n, 2]" % who)
            n, stride = int(x.shape[0]), 2
            base = x.data_ptr() if _is_device_array(x) else x.ctypes.data
            ptrs, keep = (base, base + dtype.itemsize), (x,)
        else:
            l = _check_input(left, dtype, "left", who)
            r = l if right is None else _check_input(right, dtype, "right", who)        # mono: not read
            if len(l.shape) != 1 or tuple(r.shape) != tuple(l.shape) or _is_device_array(l) != _is_device_array(r):
                raise ValueError("%s: planar input is two one-dimensional arrays of one length, in one place" % who)
            n, stride = int(l.shape[0]), 1
            ptrs = (l.data_ptr(), r.data_ptr()) if _is_device_array(l) else (l.ctypes.data, r.ctypes.data)
            keep = (l, r)
        return ptrs, stride, n, _is_device_array(keep[0]), keep

    def input_host(self):
        """The pinned host mirror of the input pool in the batch's sample type, [streams, 2, capacity] (no copy): fill it,
        then set_length(s, n) + mark_pcm(s), as with pcm_host()."""
        p = self.lib.lamehip_batch_input_host_ptr(self.b)
        if not p:
            raise RuntimeError("no pinned mirror for this batch: %s" % last_error())
        dtype = PCM_DTYPES[self.sample_type]
        buf = (C.c_char * (self.n * 2 * self.capacity * dtype.itemsize)).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(self.n, 2, self.capacity)

    def ingest_ms(self):
        """HIP-event time of the last encode()'s ingest kernel (input pool -> float pool), 0 when none ran."""
        return float(self.lib.lamehip_batch_last_ingest_ms(self.b))

    def set_replaygain(self, on=True):
        """Measure every stream's radio gain inside encode() (one kernel of its own, gain_ms()); pack_tagged() /
        get_bytes_tagged() then write it into the LAME tag.  Before encode(); not for incremental batches."""
        self.lib.lamehip_batch_set_replaygain.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_replaygain(self.b, 1 if on else 0)
        if rc:
            raise RuntimeError("lamehip_batch_set_replaygain failed (%d): %s" % (rc, last_error()))

    def set_incremental_replaygain(self, on=True):
        """ReplayGain of an incremental batch: every append*() is a call of the reference made with findReplayGain, every
        encode_available() / finish() analyses what was appended since the last round on the device; gain_windows() after any
        round, radio_gain() after finish().  Before any PCM; a converting batch needs set_incremental_resampling() first."""
        self.lib.lamehip_batch_set_incremental_replaygain.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_incremental_replaygain(self.b, 1 if on else 0)
        if rc != 0:
            raise RuntimeError("lamehip_batch_set_incremental_replaygain failed (%d): %s" % (rc, last_error()))

    def radio_gain(self, s):
        """Stream s's radio gain in tenths of a dB, as lame_get_RadioGain reports it (0: no 50 ms window completed)."""
        self.lib.lamehip_batch_radio_gain.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        v = C.c_int(0)
        rc = self.lib.lamehip_batch_radio_gain(self.b, s, C.byref(v))
        if rc:
            raise RuntimeError("lamehip_batch_radio_gain failed (%d): %s" % (rc, last_error()))
        return v.value

    def gain_windows(self, s):
        """What the gain kernel measured for stream s: float64 [windows, 2], the left and right sum of squares of every
        completed 50 ms window (test accessor)."""
        self.lib.lamehip_batch_get_gain_windows.restype = C.c_long
        self.lib.lamehip_batch_get_gain_windows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        n = self.lib.lamehip_batch_get_gain_windows(self.b, s, None, 0)
        if n < 0:
            raise RuntimeError("lamehip_batch_get_gain_windows failed (%d): %s" % (n, last_error()))
        out = np.zeros((n, 2), dtype=np.float64)
        assert self.lib.lamehip_batch_get_gain_windows(self.b, s, out.ctypes.data, n) == n
        return out

    def gain_ms(self):
        """HIP-event time of the last encode()'s gain kernel, 0 when none ran."""
        self.lib.lamehip_batch_last_gain_ms.restype = C.c_float
        self.lib.lamehip_batch_last_gain_ms.argtypes = [C.c_void_p]
        return float(self.lib.lamehip_batch_last_gain_ms(self.b))

    def set_pcm(self, s, left, right=None):
        left = np.ascontiguousarray(left, dtype=np.int16)
        right = left if right is None else np.ascontiguousarray(right, dtype=np.int16)   # mono: not read
        rc = self.lib.lamehip_batch_set_pcm(self.b, s, left.ctypes.data, right.ctypes.data, len(left))
        if rc:
            raise RuntimeError("lamehip_batch_set_pcm failed (%d): %s" % (rc, last_error()))

    def set_pcm_device(self, s, dev_left_ptr, dev_right_ptr, n):
        rc = self.lib.lamehip_batch_set_pcm_device(self.b, s, dev_left_ptr, dev_right_ptr, n)
        if rc:
            raise RuntimeError("lamehip_batch_set_pcm_device failed (%d): %s" % (rc, last_error()))

    # ---- incremental use: lame_encode_buffer semantics for all streams of the batch ----
    def append(self, s, left, right=None):
        """Stage more samples of stream s (any number, also 0); encode_available() moves everything
        staged to the GPU with one copy."""
        left = np.ascontiguousarray(left, dtype=np.int16)
        right = left if right is None else np.ascontiguousarray(right, dtype=np.int16)
        self.lib.lamehip_batch_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_append(self.b, s, left.ctypes.data, right.ctypes.data, len(left))
        if rc:
            raise RuntimeError("lamehip_batch_append failed (%d): %s" % (rc, last_error()))

    def append_input(self, s, left=None, right=None, interleaved=None):
        """More samples of stream s in the batch's sample type (any number, also 0), arguments as for set_input: planar
        `left' / `right' (right=None: mono) or one interleaved array [n, 2]; the dtype must be the batch's, nothing is
        cast.  numpy arrays are staged like append()'s shorts and leave with the next encode_available() / finish();
        arrays on the batch's GPU (data_ptr() and is_cuda, such as torch tensors) are in the pool when the call returns --
        whatever produced them must have finished.  The two may be mixed, and on a PCM_S16 batch with append()."""
        ptrs, stride, n, on_device, keep = self._input_args("append_input", left, right, interleaved)
        fn = self.lib.lamehip_batch_append_input_device if on_device else self.lib.lamehip_batch_append_input
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        rc = fn(self.b, s, ptrs[0], ptrs[1], stride, n)
        if rc:
            raise RuntimeError("lamehip_batch_append_input failed (%d): %s" % (rc, last_error()))

    def append_device(self, x, lengths):
        """One round for all streams from one array on the batch's GPU, with ONE launch: x is [B, 2, T] (planes), [B, T, 2]
        (interleaved) or, on a mono batch, [B, T]; stream s takes its first lengths[s] samples (ragged, 0 allowed).  The
        strides are the array's own (a slice x[:, :, a:b] of a larger tensor is fine), samples lie next to each other.
        Whatever produced x must have finished; it may be reused when the call returns."""
        dtype = PCM_DTYPES[self.sample_type]
        if not _is_device_array(x):
            raise TypeError("append_device: takes a device array (data_ptr() and is_cuda), append_input takes host arrays")
        name = str(x.dtype).split(".")[-1]
        if name != dtype.name:
            raise TypeError("append_device: the array is %s, the batch's sample type takes %s" % (name, dtype.name))
        shape, st = tuple(int(v) for v in x.shape), tuple(int(v) for v in x.stride())
        if len(shape) == 3 and shape[0] == self.n and shape[1] == 2:
            total, args = shape[2], (st[0], st[1], st[2])
        elif len(shape) == 3 and shape[0] == self.n and shape[2] == 2:
            total, args = shape[1], (st[0], st[2], st[1])
        elif len(shape) == 2 and shape[0] == self.n and self.enc.channels == 1:
            total, args = shape[1], (st[0], 0, st[1])
        else:
            raise ValueError("append_device: the array is [streams, 2, T], [streams, T, 2] or, on a mono batch, [streams, T]")
        if total <= 1:
            args = (args[0], args[1], 2 if args[1] == 1 else 1)         # (no second sample: its distance means nothing)
        if args[2] not in (1, 2) or (args[2] == 2 and args[1] != 1):
            raise ValueError("append_device: samples lie next to each other, or interleaved with the other plane's")
        lengths = [int(v) for v in lengths]
        if len(lengths) != self.n or min(lengths) < 0 or max(lengths) > total:
            raise ValueError("append_device: one length per stream, between 0 and what the array holds")
        n = (C.c_int * self.n)(*lengths)
        self.lib.lamehip_batch_append_device.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
        rc = self.lib.lamehip_batch_append_device(self.b, x.data_ptr(), args[0], args[1], args[2], n)
        if rc:
            raise RuntimeError("lamehip_batch_append_device failed (%d): %s" % (rc, last_error()))

    def append_ms(self):
        """HIP-event time of the append launches since, and including, the last encode_available() / finish()."""
        self.lib.lamehip_batch_last_append_ms.restype = C.c_float
        self.lib.lamehip_batch_last_append_ms.argtypes = [C.c_void_p]
        return float(self.lib.lamehip_batch_last_append_ms(self.b))

    def encode_available(self):
        """Encode every stream's newly complete frames (one launch); returns how many there were."""
        self.lib.lamehip_batch_encode_available.argtypes = [C.c_void_p]
        n = self.lib.lamehip_batch_encode_available(self.b)
        if n < 0:
            raise RuntimeError("lamehip_batch_encode_available failed (%d): %s" % (n, last_error()))
        return n

    def finish(self):
        """lame_encode_flush for every stream."""
        self.lib.lamehip_batch_finish.argtypes = [C.c_void_p]
        n = self.lib.lamehip_batch_finish(self.b)
        if n < 0:
            raise RuntimeError("lamehip_batch_finish failed (%d): %s" % (n, last_error()))
        return n

    def end_stream(self, s):
        """lame_encode_flush for stream s alone, carried out by the next encode_available() (or finish()) while the other
        streams go on; launches nothing itself.  From here on appends to s are refused until restart_stream(s)."""
        self.lib.lamehip_batch_end_stream.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_end_stream(self.b, s)
        if rc != 0:
            raise RuntimeError("lamehip_batch_end_stream failed (%d): %s" % (rc, last_error()))

    def stream_ended(self, s):
        """True behind the round that ended stream s (end_stream()), until its slot is restarted."""
        self.lib.lamehip_batch_stream_ended.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_stream_ended(self.b, s)
        if rc < 0:
            raise RuntimeError("lamehip_batch_stream_ended: no stream %d" % s)
        return bool(rc)

    def restart_stream(self, s):
        """The slot of stream s, which has ended and been drained, takes a new stream: everything of the old one is gone, the
        slot's records in HBM are put back by one launch (csrc/lh_slots.hip) at the head of the next round."""
        self.lib.lamehip_batch_restart_stream.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_restart_stream(self.b, s)
        if rc != 0:
            raise RuntimeError("lamehip_batch_restart_stream failed (%d): %s" % (rc, last_error()))

    def restart_ms(self):
        """HIP-event time of the restart launch in front of the last encode_available() / finish(); 0 when no slot was
        restarted in the gap before it."""
        self.lib.lamehip_batch_last_restart_ms.restype = C.c_float
        self.lib.lamehip_batch_last_restart_ms.argtypes = [C.c_void_p]
        return float(self.lib.lamehip_batch_last_restart_ms(self.b))

    def set_statistics(self, on=True):
        """Keep the reference's per-stream statistics (bit rate / stereo mode / block type histograms), counted on the device
        behind every encode launch (csrc/lh_stats.hip).  Before any PCM is handed over."""
        self.lib.lamehip_batch_set_statistics.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_statistics(self.b, 1 if on else 0)
        if rc != 0:
            raise RuntimeError("lamehip_batch_set_statistics failed (%d): %s" % (rc, last_error()))

    def _stat_call(self, name, *args):
        fn = getattr(self.lib, name)
        fn.argtypes = [C.c_void_p] + [C.c_int if isinstance(a, int) else C.c_void_p for a in args]
        rc = fn(self.b, *[a if isinstance(a, int) else a.ctypes.data for a in args])
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, rc, last_error()))

    def statistics(self, s):
        """(mode[16, 5], block[16, 6]) of stream s behind the last launch: mode[bitrate index | 15 = all][mode extension |
        4 = frames], block[bitrate index | 15 = all][block type 0..3 | 4 = mixed | 5 = granules]."""
        mode, block = np.zeros((16, 5), np.int32), np.zeros((16, 6), np.int32)
        self._stat_call("lamehip_batch_get_statistics", int(s), mode, block)
        return mode, block

    def statistics_all(self):
        """Every stream's tables, [B, 176]: a stream's mode[16, 5] then its block[16, 6]."""
        out = np.zeros((self.n, 176), np.int32)
        self._stat_call("lamehip_batch_get_statistics_all", out)
        return out

    def bitrate_kbps(self):
        """The bit rates that entries 0..13 of bitrate_hist() stand for."""
        out = np.zeros(14, np.int32)
        self._stat_call("lamehip_batch_bitrate_kbps", out)
        return out

    def bitrate_hist(self, s):
        """Frames of stream s per bit rate (lame_bitrate_hist)."""
        out = np.zeros(14, np.int32)
        self._stat_call("lamehip_batch_bitrate_hist", int(s), out)
        return out

    def stereo_mode_hist(self, s):
        """Frames of stream s per stereo mode: LR, LR-i, MS, MS-i (lame_stereo_mode_hist)."""
        out = np.zeros(4, np.int32)
        self._stat_call("lamehip_batch_stereo_mode_hist", int(s), out)
        return out

    def block_type_hist(self, s):
        """Granules of stream s per block type: long, start, short, stop, mixed, all (lame_block_type_hist)."""
        out = np.zeros(6, np.int32)
        self._stat_call("lamehip_batch_block_type_hist", int(s), out)
        return out

    def average_kbps(self, s):
        """sum(kbps[i] * frames[i]) / frames of stream s, the figure the reference's frontend prints; 0.0 without frames."""
        hist = self.bitrate_hist(s).astype(np.int64)
        n = int(hist.sum())
        return float((self.bitrate_kbps().astype(np.int64) * hist).sum()) / n if n else 0.0

    def stats_ms(self):
        """HIP-event time of the statistics launch behind the last encode launch; 0 when there was none."""
        self.lib.lamehip_batch_last_stats_ms.restype = C.c_float
        self.lib.lamehip_batch_last_stats_ms.argtypes = [C.c_void_p]
        return float(self.lib.lamehip_batch_last_stats_ms(self.b))

    def drain(self, s, cap=1 << 20):
        """Bytes stream s has produced since its last drain."""
        self.lib.lamehip_batch_drain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        buf = C.create_string_buffer(cap)
        k = self.lib.lamehip_batch_drain(self.b, s, buf, cap)
        if k < 0:
            raise RuntimeError("lamehip_batch_drain: buffer of %d bytes too small" % cap)
        return buf.raw[:k]

    def set_incremental_packing(self, on=True):
        """Incremental use on the device bit packer (set_device_packing() first, before any PCM): the appends are accepted,
        every encode_available() / finish() packs on the device and gathers what the streams finished into one pinned round
        buffer (csrc/lh_drain.hip); drain() copies out of it, drain_view() hands the bytes out in place."""
        self.lib.lamehip_batch_set_incremental_packing.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_incremental_packing(self.b, 1 if on else 0)
        if rc != 0:
            raise RuntimeError("lamehip_batch_set_incremental_packing failed (%d): %s" % (rc, last_error()))

    def drain_view(self, s):
        """The bytes drain(s) would return, in place (a read-only numpy view of the batch's buffer, valid until the next
        encode_available() / finish() / reset()); counts as a drain."""
        self.lib.lamehip_batch_drain_ptr.restype = C.c_long
        self.lib.lamehip_batch_drain_ptr.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_ubyte))]
        p = C.POINTER(C.c_ubyte)()
        k = self.lib.lamehip_batch_drain_ptr(self.b, s, C.byref(p))
        if k < 0:
            raise RuntimeError("lamehip_batch_drain_ptr failed (%d): %s" % (k, last_error()))
        if k == 0:
            return np.zeros(0, dtype=np.uint8)
        v = np.ctypeslib.as_array(p, shape=(k,))
        v.flags.writeable = False
        return v

    def drain_ms(self):
        """HIP-event time of the drain kernels of the last encode_available() / finish() (set_incremental_packing())."""
        self.lib.lamehip_batch_last_drain_ms.restype = C.c_float
        self.lib.lamehip_batch_last_drain_ms.argtypes = [C.c_void_p]
        return float(self.lib.lamehip_batch_last_drain_ms(self.b))

    def set_length(self, s, n):
        assert self.lib.lamehip_batch_set_length(self.b, s, n) == 0

    def pcm_device_ptr(self):
        return self.lib.lamehip_batch_pcm_device_ptr(self.b)

    def set_device_packing(self, on=True):
        """Let the kernel assemble the MP3 bytes in HBM (get_bytes) instead of leaving it to the host packer."""
        self.lib.lamehip_batch_set_device_packing.argtypes = [C.c_void_p, C.c_int]
        assert self.lib.lamehip_batch_set_device_packing(self.b, 1 if on else 0) == 0

    def set_device_tagging(self, on=True):
        """A device-packed batch (set_device_packing() first): one more kernel behind the encode kernel writes every
        stream's final tag frame in front of its bytes in HBM, and fetch() brings complete file images home -- image(),
        images_all(); get_bytes_tagged() then copies the same image.  Before encode(); may be switched between launches."""
        self.lib.lamehip_batch_set_device_tagging.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_device_tagging(self.b, 1 if on else 0)
        if rc:
            raise RuntimeError("lamehip_batch_set_device_tagging failed (%d): %s" % (rc, last_error()))

    def image(self, s):
        """Stream s's finished file image -- tag frame, then audio -- in the batch's pinned buffer (waits for fetch()); a
        uint8 view, no copy, valid until the next encode()."""
        self.lib.lamehip_batch_image_ptr.restype = C.c_long
        self.lib.lamehip_batch_image_ptr.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        p = C.c_void_p()
        k = self.lib.lamehip_batch_image_ptr(self.b, s, C.byref(p))
        if k < 0:
            raise RuntimeError("lamehip_batch_image_ptr failed (%d): %s" % (k, last_error()))
        if k == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.frombuffer((C.c_uint8 * k).from_address(p.value), dtype=np.uint8)

    def images_all(self, stride=None):
        """(buffer [B, stride] uint8, sizes) of the streams' file images."""
        if stride is None:
            stride = (max(self.frames(s) for s in range(self.n)) + 2) * 1500 + 2880
        out = np.empty((self.n, stride), dtype=np.uint8)
        sizes = np.zeros(self.n, dtype=np.int64)
        self.lib.lamehip_batch_get_images_all.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
        rc = self.lib.lamehip_batch_get_images_all(self.b, out.ctypes.data, stride, sizes.ctypes.data)
        if rc:
            raise RuntimeError("lamehip_batch_get_images_all failed (%d): %s" % (rc, last_error()))
        return out, sizes

    def bytes_device_ptr(self):
        """(device address, size) of the device packer's byte pool as the last reserve() / encode() left it (test accessor)."""
        self.lib.lamehip_batch_bytes_device_ptr.restype = C.c_void_p
        self.lib.lamehip_batch_bytes_device_ptr.argtypes = [C.c_void_p, C.c_void_p]
        n = C.c_longlong(0)
        return self.lib.lamehip_batch_bytes_device_ptr(self.b, C.byref(n)), int(n.value)

    def set_incremental_tagging(self, on=True):
        """Tag frames for an incremental batch on the device packer (set_incremental_packing() first, before any PCM): every
        round moves a carry per stream on in HBM (csrc/lh_tag.hip: lh_tag_resume_kernel), finish() brings every stream's
        final Xing/Info + LAME frame home -- tag(), tags_all().  The drains are unchanged: the caller keeps tag_size()
        bytes free at the head of the file."""
        self.lib.lamehip_batch_set_incremental_tagging.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_incremental_tagging(self.b, 1 if on else 0)
        if rc:
            raise RuntimeError("lamehip_batch_set_incremental_tagging failed (%d): %s" % (rc, last_error()))

    def tag_size(self):
        """The tag frame's length (set_incremental_tagging()); 0: the tag does not fit a frame, or the switch is off."""
        self.lib.lamehip_batch_tag_size.argtypes = [C.c_void_p]
        return int(self.lib.lamehip_batch_tag_size(self.b))

    def tag(self, s):
        """Stream s's final tag frame after finish() (set_incremental_tagging()), as bytes."""
        self.lib.lamehip_batch_tag_ptr.restype = C.c_long
        self.lib.lamehip_batch_tag_ptr.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        p = C.c_void_p()
        k = self.lib.lamehip_batch_tag_ptr(self.b, s, C.byref(p))
        if k < 0:
            raise RuntimeError("lamehip_batch_tag_ptr failed (%d): %s" % (k, last_error()))
        return C.string_at(p.value, k) if k > 0 else b""

    def tags_all(self):
        """(buffer [B, tag_size()] uint8, sizes) of the streams' tag frames after finish()."""
        stride = max(self.tag_size(), 1)
        out = np.zeros((self.n, stride), dtype=np.uint8)
        sizes = np.zeros(self.n, dtype=np.int64)
        self.lib.lamehip_batch_get_tags_all.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
        rc = self.lib.lamehip_batch_get_tags_all(self.b, out.ctypes.data, stride, sizes.ctypes.data)
        if rc:
            raise RuntimeError("lamehip_batch_get_tags_all failed (%d): %s" % (rc, last_error()))
        return out, sizes

    def tag_ms(self):
        """HIP-event time of the last encode()'s tag kernel -- with set_incremental_tagging(): of the tag launch of the last
        encode_available() / finish() --, 0 when none ran."""
        self.lib.lamehip_batch_last_tag_ms.restype = C.c_float
        self.lib.lamehip_batch_last_tag_ms.argtypes = [C.c_void_p]
        return float(self.lib.lamehip_batch_last_tag_ms(self.b))

    def set_device_resampling(self, on=True):
        """A batch whose input rate differs from the encoder's: convert on the device (inside encode()) instead of
        on the host (inside set_pcm()); opens set_pcm_device / pcm_device_ptr / set_length / pcm_host for it.
        Before any PCM is handed over."""
        self.lib.lamehip_batch_set_device_resampling.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_device_resampling(self.b, 1 if on else 0)
        if rc:
            raise RuntimeError("lamehip_batch_set_device_resampling failed (%d): %s" % (rc, last_error()))

    def set_incremental_resampling(self, on=True):
        """Incremental use of a batch that converts on the device (set_device_resampling() first): append() /
        append_input() / append_device() then take chunks at the input rate, each one call of the reference entry point,
        converter included, and encode_available() / finish() convert what came since the last round with one launch
        (resample_ms()).  Before any PCM is handed over."""
        self.lib.lamehip_batch_set_incremental_resampling.argtypes = [C.c_void_p, C.c_int]
        rc = self.lib.lamehip_batch_set_incremental_resampling(self.b, 1 if on else 0)
        if rc:
            raise RuntimeError("lamehip_batch_set_incremental_resampling failed (%d): %s" % (rc, last_error()))

    def set_stream_in_samplerate(self, s, hz):
        """Stream s arrives at hz (a batch with set_incremental_resampling(), before the stream's first sample): its bytes,
        frames, padding, tag frame and gain are those of a reference handle with in = hz and the batch's output rate given
        explicitly.  All rates of a round are converted by one launch (resample_ms()); reset() and restart_stream() put a
        stream back at the batch's own rate."""
        self.lib.lamehip_batch_set_stream_in_samplerate.argtypes = [C.c_void_p, C.c_int, C.c_int]
        rc = self.lib.lamehip_batch_set_stream_in_samplerate(self.b, s, hz)
        if rc:
            raise RuntimeError("lamehip_batch_set_stream_in_samplerate failed (%d): %s" % (rc, last_error()))

    def stream_in_samplerate(self, s):
        """The input rate of stream s: the batch's own unless set_stream_in_samplerate() stated another."""
        self.lib.lamehip_batch_stream_in_samplerate.argtypes = [C.c_void_p, C.c_int]
        hz = self.lib.lamehip_batch_stream_in_samplerate(self.b, s)
        if hz < 0:
            raise RuntimeError("lamehip_batch_stream_in_samplerate: no stream %d" % s)
        return int(hz)

    def converted(self, s):
        """The converted signal of stream s as the encoder reads it: float32 [2, converted length] (test accessor)."""
        self.lib.lamehip_batch_get_converted.restype = C.c_long
        self.lib.lamehip_batch_get_converted.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
        cap = max((self.frames(s) + 4) * 1152, self.capacity)    # (an incremental batch knows its frames at finish())
        h = getattr(self.enc, "h", None)
        rate_in, rate_out = (self.lib.lame_get_in_samplerate(h), self.lib.lame_get_out_samplerate(h)) if h else (0, 0)
        if h and hasattr(self.lib, "lamehip_batch_stream_in_samplerate"):
            rate_in = min(rate_in, self.stream_in_samplerate(s))      # (the stream's own rate, where it has one)
        if 0 < rate_in < rate_out:     # (one that converts upwards holds more than its capacity of input samples)
            cap = max(cap, self.capacity * rate_out // rate_in + 4 * 1152 + 64)
        out = np.zeros((2, cap), dtype=np.float32)
        n = self.lib.lamehip_batch_get_converted(self.b, s, out[0].ctypes.data, out[1].ctypes.data, cap)
        if n < 0:
            raise RuntimeError("lamehip_batch_get_converted failed (%d): %s" % (n, last_error()))
        return out[:, :n].copy()

    def resample_ms(self):
        """HIP-event time of the last encode()'s device conversion, 0 when none ran."""
        self.lib.lamehip_batch_last_resample_ms.restype = C.c_float
        self.lib.lamehip_batch_last_resample_ms.argtypes = [C.c_void_p]
        return float(self.lib.lamehip_batch_last_resample_ms(self.b))

    def get_bytes(self, s):
        self.lib.lamehip_batch_get_bytes.restype = C.c_long
        self.lib.lamehip_batch_get_bytes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        cap = (self.frames(s) + 2) * 1500
        buf = C.create_string_buffer(cap)
        k = self.lib.lamehip_batch_get_bytes(self.b, s, buf, cap)
        if k < 0:
            raise RuntimeError("lamehip_batch_get_bytes failed (%d): %s" % (k, last_error()))
        return buf.raw[:k]

    def get_bytes_tagged(self, s):
        self.lib.lamehip_batch_get_bytes_tagged.restype = C.c_long
        self.lib.lamehip_batch_get_bytes_tagged.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        cap = (self.frames(s) + 4) * 1500
        buf = C.create_string_buffer(cap)
        k = self.lib.lamehip_batch_get_bytes_tagged(self.b, s, buf, cap)
        if k < 0:
            raise RuntimeError("lamehip_batch_get_bytes_tagged failed (%d): %s" % (k, last_error()))
        return buf.raw[:k]

    def get_bytes_all(self, stride=None):
        """(buffer [B, stride] uint8, sizes) of the device-packed streams."""
        if stride is None:
            stride = (max(self.frames(s) for s in range(self.n)) + 2) * 1500
        out = np.empty((self.n, stride), dtype=np.uint8)
        sizes = np.zeros(self.n, dtype=np.int64)
        self.lib.lamehip_batch_get_bytes_all.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
        rc = self.lib.lamehip_batch_get_bytes_all(self.b, out.ctypes.data, stride, sizes.ctypes.data)
        if rc:
            raise RuntimeError("lamehip_batch_get_bytes_all failed (%d): %s" % (rc, last_error()))
        return out, sizes

    def pcm_host(self):
        """The pinned host mirror of the s16 pool as an int16 array [streams, 2, capacity] (no copy): fill it, then
        set_length(s, n) + mark_pcm(s); upload() / encode() move it to HBM with one asynchronous copy."""
        self.lib.lamehip_batch_pcm_host_ptr.restype = C.c_void_p
        self.lib.lamehip_batch_pcm_host_ptr.argtypes = [C.c_void_p]
        p = self.lib.lamehip_batch_pcm_host_ptr(self.b)
        if not p:
            raise RuntimeError("no pinned mirror for this batch: %s" % last_error())
        buf = (C.c_int16 * (self.n * 2 * self.capacity)).from_address(p)
        return np.frombuffer(buf, dtype=np.int16).reshape(self.n, 2, self.capacity)

    def mark_pcm(self, s):
        assert self.lib.lamehip_batch_mark_pcm(self.b, s) == 0

    def upload(self):
        rc = self.lib.lamehip_batch_upload(self.b)
        if rc:
            raise RuntimeError("lamehip_batch_upload failed (%d): %s" % (rc, last_error()))

    def fetch(self):
        """Start the device-packed bytes' way back to pinned host memory (asynchronous, behind the kernel)."""
        rc = self.lib.lamehip_batch_fetch(self.b)
        if rc:
            raise RuntimeError("lamehip_batch_fetch failed (%d): %s" % (rc, last_error()))

    def bytes_view(self, s):
        """Stream s's finished bytes in the batch's pinned buffer (waits for fetch()); a uint8 view, no copy."""
        self.lib.lamehip_batch_bytes_ptr.restype = C.c_long
        self.lib.lamehip_batch_bytes_ptr.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        p = C.c_void_p()
        k = self.lib.lamehip_batch_bytes_ptr(self.b, s, C.byref(p))
        if k < 0:
            raise RuntimeError("lamehip_batch_bytes_ptr failed (%d): %s" % (k, last_error()))
        if k == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.frombuffer((C.c_uint8 * k).from_address(p.value), dtype=np.uint8)

    def encode(self, sync=True):
        rc = self.lib.lamehip_batch_encode(self.b)
        if rc:
            raise RuntimeError("lamehip_batch_encode failed (%d): %s" % (rc, last_error()))
        if sync:
            self.sync()

    def reserve(self):
        """Allocate the launch's buffers now (payload, analysis pool) instead of in the first encode()."""
        self.lib.lamehip_batch_reserve.argtypes = [C.c_void_p]
        rc = self.lib.lamehip_batch_reserve(self.b)
        if rc:
            raise RuntimeError("lamehip_batch_reserve failed (%d): %s" % (rc, last_error()))

    def sync(self):
        rc = self.lib.lamehip_batch_sync(self.b)
        if rc:
            raise RuntimeError("lamehip_batch_sync failed (%d): %s" % (rc, last_error()))

    def reset(self):
        assert self.lib.lamehip_batch_reset(self.b) == 0

    def kernel_ms(self):
        return float(self.lib.lamehip_batch_last_kernel_ms(self.b))

    def kernel_parts_ms(self):
        """The last launch kernel by kernel: (split, [analysis, sub-band, encode] in ms); split = False: one fused kernel."""
        parts = (C.c_float * 3)()
        split = self.lib.lamehip_batch_last_kernel_parts_ms(self.b, parts)
        return bool(split == 1), [float(parts[0]), float(parts[1]), float(parts[2])]

    def windows(self):
        """Sub-launches of the last launch: 1, or the frame windows the split pipeline worked through (lamehip.h)."""
        return int(self.lib.lamehip_batch_last_windows(self.b))

    def kernel_waves(self):
        return int(self.lib.lamehip_batch_kernel_waves(self.b))

    def frames(self, s):
        return self.lib.lamehip_batch_frames(self.b, s)

    def get_frames(self, s):
        n = self.frames(s)
        arr = (LhFrameOut * n)()
        got = self.lib.lamehip_batch_get_frames(self.b, s, arr, n)
        if got != n:
            raise RuntimeError("lamehip_batch_get_frames failed (%d): %s" % (got, last_error()))
        return arr

    def pack(self, s):
        n = self.frames(s)
        buf = C.create_string_buffer(n * 1500 + 8192)
        k = self.lib.lamehip_batch_pack(self.b, s, buf, len(buf))
        if k < 0:
            raise RuntimeError("lamehip_batch_pack failed (%d): %s" % (k, last_error()))
        return buf.raw[:k]

    def pack_tagged(self, s):
        """Complete file image of stream s: final tag frame + audio frames."""
        n = self.frames(s)
        buf = C.create_string_buffer(n * 1500 + 8192 + 2880)
        self.lib.lamehip_batch_pack_tagged.restype = C.c_long
        self.lib.lamehip_batch_pack_tagged.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        k = self.lib.lamehip_batch_pack_tagged(self.b, s, buf, len(buf))
        if k < 0:
            raise RuntimeError("lamehip_batch_pack_tagged failed (%d): %s" % (k, last_error()))
        return buf.raw[:k]

    def pack_all(self, nthreads=0, as_bytes=True):
        """Pack every stream with `nthreads' host threads (0 = min(32, cores)).  Returns the list of
        mp3 byte strings, or (buffer, stride, sizes) when as_bytes is False."""
        import os
        nthreads = nthreads or min(32, os.cpu_count() or 1)
        stride = max(self.frames(s) for s in range(self.n)) * 1500 + 8192
        buf = np.empty(self.n * stride, dtype=np.uint8)
        sizes = np.zeros(self.n, dtype=np.int64)
        rc = self.lib.lamehip_batch_pack_all(self.b, nthreads, buf.ctypes.data, stride, sizes.ctypes.data)
        if rc != 0 or (sizes < 0).any():
            raise RuntimeError("lamehip_batch_pack_all failed (%d): %s" % (rc, last_error()))
        if not as_bytes:
            return buf, stride, sizes
        return [buf[s * stride: s * stride + int(sizes[s])].tobytes() for s in range(self.n)]

    def close(self):
        if self.b:
            self.lib.lamehip_batch_destroy(self.b)
            self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_streams(total_streams, world_size, rank):
    """Static sharding of a batch of independent streams over the GPUs of a node:
    rank r of world_size owns the contiguous block [lo, hi) of global stream indices; blocks differ
    by at most one stream and cover the batch exactly.  No collective is involved anywhere on the
    data path -- a stream's state never leaves its device."""
    if world_size <= 0 or not (0 <= rank < world_size) or total_streams < 0:
        raise ValueError("shard_streams(%r, %r, %r)" % (total_streams, world_size, rank))
    base, extra = divmod(total_streams, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)
