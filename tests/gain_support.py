"""What the tests of a batch's ReplayGain share (test_batch_replaygain.py, test_batch_replaygain_device.py): ctypes
bindings of the host plan and the host twin (csrc/lh_replaygain.c), the records of a launch (csrc/lh_gain.h), the blocks the
handle API hands to its analysis restated in Python -- independently of lh_gain_plan --, and the settings and lengths."""
import ctypes as C

import numpy as np

import helpers
import lamehip
import resample_support as rsup

MF_START = 528
RATES = [48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000]


class LhReplayGain(C.Structure):
    _fields_ = [("rate_index", C.c_int), ("window", C.c_long), ("filled", C.c_long), ("lsum", C.c_double), ("rsum", C.c_double),
                ("hist", (C.c_float * 10) * 6), ("bins", C.c_uint32 * 12000), ("work", (C.c_float * (10 + 2404)) * 3)]


class LhGainStream(C.Structure):
    _fields_ = [("n", C.c_longlong), ("win_at", C.c_longlong), ("total", C.c_int), ("stream", C.c_int), ("ntrunk", C.c_int),
                ("tail_at", C.c_int), ("ntail", C.c_int), ("pad_", C.c_int)]


class LhGainParams(C.Structure):
    _fields_ = [("m", C.c_float * 4), ("ky", C.c_float * 21), ("kb", C.c_float * 5), ("cap", C.c_longlong), ("window", C.c_int),
                ("fs", C.c_int), ("channels", C.c_int), ("one_plane", C.c_int), ("taps", C.c_int)]


# name, input rate, output rate, channels of the encoder, input planes, scale, sample type, frame size
#   channels 1 / planes 2: mono downmixed from stereo (the frontend's -a: both planes at half weight, times the scale)
SETTINGS = [
    ("44k1-stereo", 44100, 44100, 2, 2, 1.0, "s16", 1152),
    ("48k-joint", 48000, 48000, 2, 2, 1.0, "s16", 1152),
    ("32k-mono", 32000, 32000, 1, 1, 1.0, "s16", 1152),
    ("44k1-downmix-0.6", 44100, 44100, 1, 2, 0.6, "s16", 1152),
    ("22k05-mpeg2", 22050, 22050, 2, 2, 1.0, "s16", 576),
    ("f32-48k-to-44k1", 48000, 44100, 2, 2, 1.0, "f32unit", 1152),
    ("s16-44k1-to-32k", 44100, 32000, 2, 2, 1.0, "s16", 1152),
]


def window_of(rate):
    return (rate + 19) // 20


def lengths_of(rate_in, rate_out, fs):
    """the lengths every setting is tested at, in input samples: around ten samples (a block's first piece), a frame, a
    window W at the output rate and their multiples, and about 0.7 s"""
    w = window_of(rate_out)
    return [0, 1, 9, 10, 11, fs - 1, fs, fs + 1, w - 1, w, w + 1, w + 10, 2 * w, 3 * fs, int(0.7 * rate_in)]


def library():
    lib = rsup.library()
    lib.lh_rg_start.argtypes = [C.c_void_p, C.c_int]
    lib.lh_rg_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.lh_rg_finish.argtypes = [C.c_void_p]
    lib.lh_gain_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    lib.lh_gain_eval_host.restype = C.c_long
    lib.lh_gain_eval_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p,
                                      C.c_long, C.c_void_p]
    lib.lh_gain_from_windows.argtypes = [C.c_void_p, C.c_long, C.c_long]
    return lib


def plan(lib, rs, fs, n):
    """lh_gain_plan: (block lengths, samples heard); rs: an initialised LhResampler, or None"""
    mfn = 1024 + fs - 272
    total = C.c_long(-1)
    k = lib.lh_gain_plan(C.byref(rs) if rs is not None else None, fs, mfn, n, None, 0, C.byref(total))
    assert k >= 0
    blocks = (C.c_int * max(k, 1))()
    assert lib.lh_gain_plan(C.byref(rs) if rs is not None else None, fs, mfn, n, blocks, k, C.byref(total)) == k
    return list(blocks[:k]), total.value


def eval_host(lib, rate, channels, blocks, x):
    """lh_gain_eval_host on float32 planes x [2, n]: (window sums float64 [windows, 2], tenths of a dB)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[1]
    arr = (C.c_int * max(len(blocks), 1))(*blocks)
    cap = sum(blocks) // window_of(rate) + 1
    pairs = np.full((cap, 2), -1.0, np.float64)
    tenths = C.c_int(-99999)
    k = lib.lh_gain_eval_host(rate, channels, arr, len(blocks), x[0].ctypes.data, x[1].ctypes.data, n, pairs.ctypes.data, cap,
                              C.byref(tenths))
    assert 0 <= k < cap
    return pairs[:k].copy(), tenths.value


def same_doubles(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def signal(setting, seed, n, amp=1.0):
    """n input samples of a setting in its sample type ([2, n]; a mono setting reads plane 0 alone)"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    x = helpers.synth_stream(seed, max(n, 1), rate_in)[:, :n]
    x = (x.astype(np.float64) * amp).astype(np.int16)
    if stype == "f32unit":
        return (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    return x


def heard(setting, x):
    """what the encoder makes of input x before any rate conversion: float32 [2, n] behind the PCM matrix, every product and
    sum a float32 (lame_copy_inbuffer); plane 1 of a mono setting is not part of the analysis"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    f = np.float32
    norm = f(32767.0) if stype == "f32unit" else f(1.0)
    xl, xr = x[0].astype(np.float32), x[1].astype(np.float32)
    if channels == 2:
        return np.stack([xl * (norm * f(scale)), xr * (norm * f(scale))]).astype(np.float32)
    if planes == 2:     # downmix: 0.5 * scale on both planes
        h = norm * (f(0.5) * f(scale))
        u = ((xl * h).astype(np.float32) + (xr * h).astype(np.float32)).astype(np.float32)
        return np.stack([u, np.zeros_like(u)])
    return np.stack([(xl * (norm * f(scale))).astype(np.float32), np.zeros_like(xl)])


class HandleBlocks:
    """The blocks lame_encode_buffer / lame_encode_flush of the handle API hand to lh_rg_block for a stream fed `fs' input
    samples per call (csrc/lh_api.cpp: encode_buffer_impl, lame_encode_flush, flush_resampled), restated on the host alone:
    `blocks' is the list of float32 [2, made] arrays, in order."""

    def __init__(self, lib, setting, y):
        name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
        self.lib, self.fs, self.mfn, self.channels = lib, fs, 1024 + fs - 272, channels
        self.rs = rsup.resampler(lib, rate_in, rate_out) if rate_in != rate_out else None
        self.blocks, self.fed, self.frames = [], 0, 0
        n = y.shape[1]
        for at in range(0, n, fs):
            self.feed(y[:, at:at + fs])
        if self.rs is None:
            owed = 576 + self.fed - fs * self.frames
            padding = fs - owed % fs
            if padding < 576:
                padding += fs
            left = (owed + padding) // fs
            fed, frames = self.fed, self.frames
            while left > 0:
                bunch = min(1152, max(1, self.mfn - (MF_START + fed - fs * frames)))
                self.blocks.append(np.zeros((2, bunch), np.float32))
                fed += bunch
                if MF_START + fed - fs * frames >= self.mfn:
                    frames += 1
                    left -= 1
        else:
            ratio = self.rs.ratio
            owed = int(576 + self.fed - fs * self.frames + 16.0 / ratio)
            padding = fs - owed % fs
            if padding < 576:
                padding += fs
            left = (owed + padding) // fs
            while left > 0:
                before = self.frames
                bunch = int((self.mfn - (MF_START + self.fed - fs * self.frames)) * ratio)
                bunch = min(1152, max(1, bunch))
                self.feed(np.zeros((2, bunch), np.float32))
                left -= 1 if self.frames != before else 0

    def feed(self, chunk):
        """one lame_encode_buffer call"""
        chunk = np.ascontiguousarray(chunk, dtype=np.float32)
        n = chunk.shape[1]
        if n == 0:
            return
        if self.rs is None:
            for at in range(0, n, self.fs):
                self.blocks.append(chunk[:, at:at + self.fs].copy())
            self.fed += n
        else:
            pos = 0
            while pos < n:
                blk = np.zeros((2, 1152), np.float32)
                used, made = C.c_int(0), 0
                for ch in range(self.channels):
                    made = self.lib.lh_rs_block(C.byref(self.rs), ch, blk[ch].ctypes.data, self.fs, chunk[ch, pos:].ctypes.data,
                                                n - pos, C.byref(used))
                self.blocks.append(blk[:, :made].copy())
                self.fed += made
                pos += used.value
        if MF_START + self.fed >= self.mfn:
            self.frames = (MF_START + self.fed - self.mfn) // self.fs + 1

    def signal(self):
        return np.concatenate(self.blocks, axis=1) if self.blocks else np.zeros((2, 0), np.float32)


def block_by_block(lib, rate, channels, blocks, ref=None):
    """lh_rg_block / lh_rg_finish fed `blocks' (float32 [2, n] each): (bins as a tuple of (bin, count), tenths); with `ref'
    (the compiled reference's library) also AnalyzeSamples / GetTitleGain fed the same: (..., tenths of the reference)"""
    g = LhReplayGain()
    assert lib.lh_rg_start(C.byref(g), rate) == 0
    theirs = None
    if ref is not None:
        theirs = C.create_string_buffer(400000)
        ref.InitGainAnalysis.argtypes = [C.c_void_p, C.c_long]
        ref.AnalyzeSamples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        ref.GetTitleGain.restype = C.c_float
        ref.GetTitleGain.argtypes = [C.c_void_p]
        assert ref.InitGainAnalysis(theirs, rate) == 1
    for b in blocks:
        l, r = np.ascontiguousarray(b[0]), np.ascontiguousarray(b[1])
        if len(l) == 0:
            continue
        assert lib.lh_rg_block(C.byref(g), l.ctypes.data, r.ctypes.data, len(l), channels) == 0
        if theirs is not None:
            assert ref.AnalyzeSamples(theirs, l.ctypes.data, r.ctypes.data, len(l), channels) == 1
    bins = np.frombuffer(g.bins, dtype=np.uint32).copy()
    hist = tuple((int(i), int(bins[i])) for i in np.nonzero(bins)[0])
    tenths = lib.lh_rg_finish(C.byref(g))
    if theirs is None:
        return hist, tenths
    want = ref.GetTitleGain(theirs)
    # (reference lame.c:1571-1578: the float gain times ten and the rounding are double arithmetic)
    return hist, tenths, (0 if want == -24601 else int(np.floor(float(np.float32(want)) * 10.0 + 0.5)))


def bins_of(lib, pairs, window):
    """the histogram lh_rg_bin (the text lh_rg_block itself files a finished window with) makes of window sums"""
    lib.lh_rg_bin.restype = C.c_size_t
    lib.lh_rg_bin.argtypes = [C.c_double, C.c_double, C.c_long]
    hist = {}
    for l, r in pairs:
        b = int(lib.lh_rg_bin(float(l), float(r), window))
        hist[b] = hist.get(b, 0) + 1
    return tuple(sorted(hist.items()))


# ---- on the device: handles and batches of a setting ----

def open_handle(setting, find_gain=False, write_tag=False, vbr_q=None):
    """a handle with a setting's parameters; find_gain: lame_set_findReplayGain(1), what the frontend does by default"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    enc = lamehip.Encoder.__new__(lamehip.Encoder)
    lib = enc.lib = lamehip.load_library()
    enc.h = C.c_void_p(lib.lame_init())
    enc.channels = planes
    lib.lame_set_in_samplerate(enc.h, rate_in)
    if rate_out != rate_in:
        lib.lame_set_out_samplerate(enc.h, rate_out)
    lib.lame_set_num_channels(enc.h, planes)
    lib.lame_set_bWriteVbrTag(enc.h, 1 if write_tag else 0)
    if vbr_q is not None:
        lib.lame_set_VBR(enc.h, 4)
        lib.lame_set_VBR_q(enc.h, vbr_q)
    else:
        lib.lame_set_brate(enc.h, 64 if fs == 576 else 128)
    if name == "48k-joint":
        lib.lame_set_mode(enc.h, 1)
    if channels == 1 and planes == 2:
        lib.lame_set_mode(enc.h, 3)
    if scale != 1.0:
        lib.lame_set_scale.argtypes = [C.c_void_p, C.c_float]
        lib.lame_set_scale(enc.h, scale)
    if find_gain:
        lib.lame_set_findReplayGain(enc.h, 1)
    enc.rc = lib.lame_init_params(enc.h)
    assert enc.rc == 0, lamehip.last_error()
    return enc


def handle_stream(enc, setting, x):
    """stream x through the handle, a frame's worth of input samples per call, then the flush: (bytes, lame_get_RadioGain)"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    lib = enc.lib
    fn = lib.lame_encode_buffer_ieee_float if stype == "f32unit" else lib.lame_encode_buffer
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lame_get_RadioGain.argtypes = [C.c_void_p]
    buf = C.create_string_buffer(4 * fs + 16000)
    out = b""
    for at in range(0, x.shape[1], fs):
        l, r = np.ascontiguousarray(x[0, at:at + fs]), np.ascontiguousarray(x[1 if planes == 2 else 0, at:at + fs])
        k = fn(enc.h, l.ctypes.data, r.ctypes.data, len(l), buf, len(buf))
        assert k >= 0
        out += buf.raw[:k]
    k = lib.lame_encode_flush(enc.h, buf, len(buf))
    assert k >= 0
    return out + buf.raw[:k], lib.lame_get_RadioGain(enc.h)


def make_batch(enc, setting, nstreams, cap, packing=False):
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    b = lamehip.Batch(enc, nstreams, cap)
    if packing:
        b.set_device_packing()
    if rate_in != rate_out:
        b.set_device_resampling()
    if stype == "f32unit":
        b.set_sample_type(lamehip.PCM_F32_UNIT)
    return b


def feed_batch(b, setting, xs):
    """host arrays through set_pcm / set_input"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    for s, x in enumerate(xs):
        if stype == "f32unit":
            b.set_input(s, x[0], x[1] if planes == 2 else None)
        else:
            b.set_pcm(s, x[0], x[1] if planes == 2 else None)


def feed_batch_in_place(b, setting, xs, cap):
    """device-resident input: the whole pool written through pcm_device_ptr -- the setting's poison (s16 0x7fff, float NaN)
    at and beyond every stream's length, and all over the plane a mono setting never reads --, then the lengths declared"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    lib = b.lib
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.full((len(xs), 2, cap), np.nan, np.float32) if stype == "f32unit" else np.full((len(xs), 2, cap), 0x7fff, np.int16)
    for s, x in enumerate(xs):
        host[s, :planes, :x.shape[1]] = x[:planes]
    assert lib.hipMemcpy(b.pcm_device_ptr(), host.ctypes.data, host.nbytes, 1) == 0     # 1 = hipMemcpyHostToDevice
    for s, x in enumerate(xs):
        b.set_length(s, x.shape[1])


def heard_by_batch(b, enc, setting, s, x):
    """the samples of stream s as the encoder reads them: float32 [2, n] -- converted() where the batch has a float pool,
    else the s16 samples behind the PCM matrix, every product and sum a float32"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    if rate_in != rate_out or stype != "s16":
        return b.converted(s)
    cfg = enc.config()
    f = np.float32
    m00, m01, m10, m11 = f(cfg.pcm_scale), f(cfg.pcm_mix), f(0.0) * f(cfg.pcm_scale), f(cfg.pcm_scale_r)
    xl = x[0].astype(np.float32)
    xr = x[1 if planes == 2 else 0].astype(np.float32)
    u = ((xl * m00).astype(np.float32) + (xr * m01).astype(np.float32)).astype(np.float32)
    v = ((xl * m10).astype(np.float32) + (xr * m11).astype(np.float32)).astype(np.float32)
    return np.stack([u, v])


def expected_of_stream(lib, b, enc, setting, s, x):
    """the host twin on what the batch's encoder reads: (window sums, tenths of a dB)"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    rs = rsup.resampler(lib, rate_in, rate_out) if rate_in != rate_out else None
    blocks, total = plan(lib, rs, fs, x.shape[1])
    return eval_host(lib, rate_out, channels, blocks, heard_by_batch(b, enc, setting, s, x))
