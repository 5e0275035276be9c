"""ReplayGain of an incremental batch (lamehip_batch_set_incremental_replaygain): ctypes bindings of the plan that follows the
calls (csrc/lh_replaygain.c: lh_gain_plan_call, lh_gain_plan_flush) and of a stream's carry (csrc/lh_gain.h), the handle's
calls restated in Python -- gain_support.HandleBlocks driven call by call, then its flush --, the host twin's own state behind
a list of blocks, and the lists of calls and rounds, for test_append_replaygain_plan.py and test_append_replaygain_device.py."""
import ctypes as C
import os
import random
import re

import numpy as np

import append_resample_support as ars
import gain_support as gs
import helpers
import resample_support as rsup

MF_START = gs.MF_START


class LhGainCursor(C.Structure):
    _fields_ = [("heard", C.c_longlong), ("fed", C.c_longlong), ("frames", C.c_long)]

    def key(self):
        return (self.heard, self.fed, self.frames)


class LhGainCarry(C.Structure):
    _fields_ = [("x", (C.c_float * 10) * 2), ("mid", (C.c_float * 10) * 2), ("out", (C.c_float * 2) * 2), ("lsum", C.c_double),
                ("rsum", C.c_double), ("heard", C.c_longlong), ("windows", C.c_longlong)]


def library():
    lib = gs.library()
    ars.library()               # (the same library object: the conversion's call plan)
    lib.lh_gain_cursor_init.argtypes = [C.c_void_p]
    lib.lh_gain_cursor_init.restype = None
    lib.lh_gain_plan_call.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.lh_gain_plan_flush.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return lib


def call_lengths(setting):
    """the lengths the calls of every test are made of, in input samples"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    w = gs.window_of(rate_out)
    return [0, 1, 9, 10, 11, fs - 1, fs, fs + 1, w - 1, w, w + 1, 3 * fs + 7]


def call_orders(setting, seed=7):
    """chunk lists of those lengths: as listed, backwards, every fifth, shuffled, and a short one that ends on a 0"""
    ls = call_lengths(setting)
    rnd = random.Random(seed)
    shuffled = ls[:]
    rnd.shuffle(shuffled)
    return [ls, ls[::-1], [ls[(5 * i + 3) % len(ls)] for i in range(len(ls))], shuffled, [ls[8], ls[3], ls[1], ls[0]]]


def into_rounds(calls, seed):
    """a list of calls grouped into rounds of 0 to 3 calls, in order"""
    rnd, rounds, at = random.Random(seed), [], 0
    while at < len(calls):
        k = rnd.randint(0, 3)
        rounds.append(calls[at:at + k])
        at += k
    return rounds


class CallPlan:
    """the plan of one stream that follows the calls: lh_gain_plan_call / _flush, or -- a converting setting -- the made counts
    of lh_rs_plan_call / _flush with the blocks that make nothing dropped (what lh_batch.cpp hands the kernel)"""

    def __init__(self, lib, setting):
        name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
        self.lib, self.fs, self.mfn = lib, fs, 1024 + fs - 272
        self.rs = rsup.resampler(lib, rate_in, rate_out) if rate_in != rate_out else None
        if self.rs is None:
            self.cur = LhGainCursor(-1, -1, -1)
            lib.lh_gain_cursor_init(C.byref(self.cur))
        else:
            self.cur = ars.cursor(lib)

    def heard(self):
        return self.cur.heard if self.rs is None else self.cur.fed

    def call(self, m):
        if self.rs is not None:
            return [b.made for b in ars.plan_call(self.lib, self.rs, self.cur, m) if b.made > 0]
        return self._twice(lambda cur, blocks, cap: self.lib.lh_gain_plan_call(cur, self.fs, self.mfn, m, blocks, cap))

    def flush(self):
        if self.rs is not None:
            return [b.made for b in ars.plan_flush(self.lib, self.rs, self.cur)[0] if b.made > 0]
        return self._twice(lambda cur, blocks, cap: self.lib.lh_gain_plan_flush(cur, self.fs, self.mfn, blocks, cap))

    def _twice(self, fn):
        """counted with no room, then written: the same count, the same cursor, nothing beyond the room"""
        probe = LhGainCursor.from_buffer_copy(self.cur)
        n = fn(C.byref(probe), None, 0)
        assert n >= 0
        blocks = (C.c_int * (n + 1))(*([-7] * (n + 1)))
        assert fn(C.byref(self.cur), blocks, n) == n
        assert probe.key() == self.cur.key() and blocks[n] == -7
        return list(blocks[:n])


class Calls(gs.HandleBlocks):
    """gain_support.HandleBlocks fed by the caller: feed() is one lame_encode_buffer call of any length, flush() is
    lame_encode_flush (csrc/lh_api.cpp) restated as HandleBlocks restates it behind calls of one frame"""

    def __init__(self, lib, setting):
        name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
        self.lib, self.fs, self.mfn, self.channels = lib, fs, 1024 + fs - 272, channels
        self.rs = rsup.resampler(lib, rate_in, rate_out) if rate_in != rate_out else None
        self.blocks, self.fed, self.frames = [], 0, 0

    def flush(self):
        fs = self.fs
        ratio = self.rs.ratio if self.rs is not None else None
        owed = 576 + self.fed - fs * self.frames
        if ratio is not None:
            owed = int(owed + 16.0 / ratio)
        padding = fs - owed % fs
        if padding < 576:
            padding += fs
        left = (owed + padding) // fs
        while left > 0:
            before = self.frames
            bunch = self.mfn - (MF_START + self.fed - fs * self.frames)
            if ratio is not None:
                bunch = int(bunch * ratio)
            bunch = min(1152, max(1, bunch))
            if ratio is None:
                # (lame_encode_flush counts its frames by the buffer, one bunch may not complete one)
                self.blocks.append(np.zeros((2, bunch), np.float32))
                self.fed += bunch
                if MF_START + self.fed - fs * self.frames >= self.mfn:
                    self.frames += 1
            else:
                self.feed(np.zeros((2, bunch), np.float32))
            left -= 1 if self.frames != before else 0

    def lengths(self, first=0):
        return [b.shape[1] for b in self.blocks[first:] if b.shape[1] > 0]


def twin_state(lib, rate, channels, blocks, x):
    """lh_rg_block over `blocks' (lengths) cut from x [2, n] (zeros from n on), stopped before lh_rg_finish: the LhReplayGain"""
    g = gs.LhReplayGain()
    assert lib.lh_rg_start(C.byref(g), rate) == 0
    total = sum(blocks)
    y = np.zeros((2, total), np.float32)
    k = min(total, x.shape[1])
    y[:, :k] = x[:, :k]
    at = 0
    for m in blocks:
        l, r = np.ascontiguousarray(y[0, at:at + m]), np.ascontiguousarray(y[1, at:at + m])
        assert lib.lh_rg_block(C.byref(g), l.ctypes.data, r.ctypes.data, m, channels) == 0
        at += m
    return g


def carry_matches(carry, g, channels, heard, windows):
    """a stream's carry against the twin's state behind the same blocks: None, or what differs"""
    f = lambda a: np.array(a, dtype=np.float32).tobytes()
    for c in range(1 if channels == 1 else 2):
        if f(carry.x[c]) != f(g.hist[c]):
            return "inputs of channel %d" % c
        if f(carry.mid[c]) != f(g.hist[2 + c]):
            return "first filter's outputs of channel %d" % c
        if f(carry.out[c]) != f(g.hist[4 + c][8:10]):
            return "second filter's outputs of channel %d" % c
    if np.float64(carry.lsum).tobytes() != np.float64(g.lsum).tobytes() or np.float64(carry.rsum).tobytes() != np.float64(g.rsum).tobytes():
        return "open window's sums"
    if carry.heard != heard or carry.heard % g.window != g.filled:
        return "samples heard"
    if carry.windows != windows:
        return "windows finished"
    return None


def filter_rows(rate):
    """the rate's rows of csrc/lh_replaygain_tables.h, read from the header (the library does not export them)"""
    text = open(os.path.join(helpers.PKG, "csrc", "lh_replaygain_tables.h")).read()
    rows = {}
    for name, width in (("lh_rg_yule", 21), ("lh_rg_butter", 5)):
        body = text[text.index(name):]
        body = body[body.index("{") + 1:body.index("};")]
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        vals = [float(v.rstrip("fF")) for v in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?[fF]?|[-+]?\d+\.?(?:[eE][-+]?\d+)?[fF]?", body)]
        assert len(vals) == 9 * width, (name, len(vals))
        rows[name] = np.array(vals, np.float64).astype(np.float32).reshape(9, width)[gs.RATES.index(rate)]
    return list(rows["lh_rg_yule"]), list(rows["lh_rg_butter"])


# ---- on the device ----

class DevArray:
    """a numpy array copied to HBM (hipMalloc through the library), as Batch.append_input / append_device take device arrays:
    data_ptr(), is_cuda, dtype, shape, stride() in elements -- what a torch tensor says of itself, without torch"""
    is_cuda = True

    def __init__(self, lib, host):
        host = np.ascontiguousarray(host)
        self.lib, self.dtype, self.shape = lib, host.dtype, host.shape
        self._strides = tuple(st // host.itemsize for st in host.strides)
        lib.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
        lib.hipFree.argtypes = [C.c_void_p]
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.p = C.c_void_p()
        assert lib.hipMalloc(C.byref(self.p), max(host.nbytes, 16)) == 0
        if host.nbytes:
            assert lib.hipMemcpy(self.p, host.ctypes.data, host.nbytes, 1) == 0     # 1 = hipMemcpyHostToDevice

    def data_ptr(self):
        return self.p.value

    def stride(self):
        return self._strides

    def is_contiguous(self):
        return True

    def free(self):
        if self.p:
            self.lib.hipFree(self.p)
        self.p = C.c_void_p()


def calls_of(setting, s, n):
    """stream s of n input samples cut into calls of call_lengths(setting), the order varying with s; the last one is what is left"""
    order = call_orders(setting)[s % 5]
    calls, at, i = [], 0, s
    while at < n:
        m = min(order[i % len(order)], n - at)
        calls.append(m)
        at += m
        i += 1
    return calls if calls else [0]


def open_inc_batch(enc, setting, nstreams, cap, switch=True):
    """an incremental batch of a setting: the converter round by round where it converts, the gain round by round with `switch'"""
    import lamehip
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    b = lamehip.Batch(enc, nstreams, cap)
    if rate_in != rate_out:
        b.set_device_resampling()
    if stype == "f32unit":
        b.set_sample_type(lamehip.PCM_F32_UNIT)
    if rate_in != rate_out:
        b.set_incremental_resampling()
    if switch:
        b.set_incremental_replaygain()
    return b


def append_call(b, setting, s, x, how, keep):
    """one call of stream s: x [2, m] of the setting's type; how 0: lamehip_batch_append (s16) / append_input from host arrays,
    1: append_input from host arrays (interleaved where the setting has two planes), 2: append_input from device arrays"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    l, r = np.ascontiguousarray(x[0]), (np.ascontiguousarray(x[1]) if planes == 2 else None)
    if how == 2:
        dl = DevArray(b.lib, l)
        dr = DevArray(b.lib, r) if r is not None else None
        b.append_input(s, dl, dr)
        keep += [dl] + ([dr] if dr is not None else [])
    elif how == 1 and r is not None:
        b.append_input(s, interleaved=np.ascontiguousarray(x.T))
    elif how == 0 and stype == "s16":
        b.append(s, l, r)
    else:
        b.append_input(s, l, r)


def handle_calls(setting, x, calls):
    """stream x through a handle with lame_set_findReplayGain(1), one lame_encode_buffer* call per entry of `calls', then the
    flush: (bytes, lame_get_RadioGain)"""
    name, rate_in, rate_out, channels, planes, scale, stype, fs = setting
    enc = gs.open_handle(setting, find_gain=True)
    lib = enc.lib
    fn = lib.lame_encode_buffer_ieee_float if stype == "f32unit" else lib.lame_encode_buffer
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lame_get_RadioGain.argtypes = [C.c_void_p]
    buf = C.create_string_buffer(2 * max(calls + [fs]) + 16000)
    out, at = b"", 0
    for m in calls:
        l, r = np.ascontiguousarray(x[0, at:at + m]), np.ascontiguousarray(x[1 if planes == 2 else 0, at:at + m])
        k = fn(enc.h, l.ctypes.data, r.ctypes.data, m, buf, len(buf))
        assert k >= 0
        out += buf.raw[:k]
        at += m
    k = lib.lame_encode_flush(enc.h, buf, len(buf))
    assert k >= 0
    gain = lib.lame_get_RadioGain(enc.h)
    enc.close()
    return out + buf.raw[:k], gain


class Twin:
    """the host twin of one stream of a batch, following its calls: the blocks so far (CallPlan) and, on demand, the windows
    lh_gain_eval_host makes of them over what the batch's encoder has read so far"""

    def __init__(self, lib, setting):
        self.lib, self.setting, self.cp, self.blocks = lib, setting, CallPlan(lib, setting), []

    def call(self, m):
        self.blocks += self.cp.call(m)

    def flush(self):
        self.blocks += self.cp.flush()

    def windows(self, b, enc, s, x_fed):
        """x_fed: the input handed over so far, [2, n]; (window sums, tenths)"""
        name, rate_in, rate_out, channels, planes, scale, stype, fs = self.setting
        heard = gs.heard_by_batch(b, enc, self.setting, s, x_fed)
        if rate_in != rate_out:
            assert heard.shape[1] == sum(self.blocks), "stream %d: the pool holds %d samples, the plan %d" % (s, heard.shape[1], sum(self.blocks))
        else:
            heard = heard[:, :x_fed.shape[1]]
        return gs.eval_host(self.lib, rate_out, channels, self.blocks, heard)
