"""What the batch statistics tests share (tests/test_batch_stats.py, tests/test_batch_stats_device.py): expected values that
do not come from the code under test.  A small parser of an MP3 byte stream -- header and side info only -- gives, per frame,
what the reference's updateStats counts (encoder.c:156-184): the bit rate index, the mode extension and the block type of
every granule and channel (4 for a mixed block); hist() makes the two tables of any run of frames from these keys."""
import numpy as np

KBPS = {1: (0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320),
        0: (0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160)}
RATES = {3: (44100, 48000, 32000), 2: (22050, 24000, 16000), 0: (11025, 12000, 8000)}

# the fixtures of the statistics tests: what the reference's own bytes give for them (asserted from the parse before anything
# is compared, so that no test passes on empty bins): frames, distinct bit rates, (LR, MS) frames or None for mono, granules
# per block type 0..3
FIXTURES = {
    "vbr2_js_44k": (59, 6, (7, 52), (196, 12, 16, 12)),
    "abr56_js_22k_lsf": (41, 9, (0, 41), (48, 10, 14, 10)),
    "mono_vbr2_44k": (40, 7, None, (64, 5, 6, 5)),
    "cbr16_js_8k_lsf": (23, 1, (1, 22), (16, 8, 16, 6)),
    "vbrold0_js_48k_bursts": (35, 3, (34, 1), (2, 2, 134, 2)),
    "cbr192_st_44k": (40, 1, (40, 0), (128, 10, 12, 10)),
}
LSF = ("abr56_js_22k_lsf", "cbr16_js_8k_lsf")
NT = 256                                        # LH_STATS_NT (csrc/lh_stats.hip): lanes of the kernel's workgroup


class Bits:
    def __init__(self, data, at):
        self.data, self.pos = data, at * 8

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.data[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v


def parse(mp3):
    """[(bitrate index, mode extension, (block type bin per granule and channel, granule-major))] per frame, and
    (channels, granules per frame).  Every byte of the stream must belong to a frame."""
    mp3 = bytes(mp3)
    keys, at, shape = [], 0, None
    while at < len(mp3):
        assert at + 4 <= len(mp3), "half a header at %d" % at
        h = mp3[at:at + 4]
        assert h[0] == 0xFF and (h[1] & 0xE0) == 0xE0 and ((h[1] >> 1) & 3) == 1, "no layer III header at %d" % at
        ver = (h[1] >> 3) & 3
        assert ver in RATES, "reserved version at %d" % at
        mpeg1, protected = ver == 3, (h[1] & 1) == 0
        bi, sri, pad = h[2] >> 4, (h[2] >> 2) & 3, (h[2] >> 1) & 1
        assert 1 <= bi <= 14 and sri < 3, "free format or bad index at %d" % at
        channels, me = (1 if (h[3] >> 6) == 3 else 2), (h[3] >> 4) & 3
        kbps, rate = KBPS[1 if mpeg1 else 0][bi], RATES[ver][sri]
        length = (144000 if mpeg1 else 72000) * kbps // rate + pad
        ngr = 2 if mpeg1 else 1
        assert shape in (None, (channels, ngr)), "the stream changes shape at %d" % at
        shape = (channels, ngr)
        r = Bits(mp3, at + 4 + (2 if protected else 0))
        if mpeg1:
            r.get(9)
            r.get(5 if channels == 1 else 3)
            r.get(4 * channels)
        else:
            r.get(8)
            r.get(1 if channels == 1 else 2)
        bts = []
        for _gr in range(ngr):
            for _ch in range(channels):
                r.get(12)
                r.get(9)
                r.get(8)
                r.get(4 if mpeg1 else 9)
                if r.get(1):
                    bt = r.get(2)
                    mixed = r.get(1)
                    r.get(19)
                    bts.append(4 if mixed else bt)
                else:
                    r.get(22)
                    bts.append(0)
                r.get(3 if mpeg1 else 2)
        assert r.pos <= (at + length) * 8
        keys.append((bi, me, tuple(bts)))
        at += length
    assert at == len(mp3), "the last frame is cut short"
    return keys, (shape or (2, 2))


def hist(keys, channels):
    """(mode[16, 5], block[16, 6]) of the frames `keys', the rule of updateStats"""
    mode, block = np.zeros((16, 5), np.int32), np.zeros((16, 6), np.int32)
    for bi, me, bts in keys:
        for row in (bi, 15):
            mode[row][4] += 1
            if channels == 2:
                mode[row][me] += 1
            for bt in bts:
                block[row][bt] += 1
                block[row][5] += 1
    return mode, block


def flat(mode, block):
    """the 176 ints of an LhStatCarry"""
    return np.concatenate([np.asarray(mode, np.int32).ravel(), np.asarray(block, np.int32).ravel()])


def check_fixture_facts(name, keys, channels, ngr):
    """the table of the fixtures: the parse of the golden bytes has what the tests rely on"""
    frames, rates, lr_ms, bt = FIXTURES[name]
    mode, block = hist(keys, channels)
    assert len(keys) == frames == mode[15][4]
    assert int((mode[1:15, 4] > 0).sum()) == rates
    if lr_ms is None:
        assert channels == 1 and not mode[:, :4].any()
    else:
        assert (int(mode[15][0]), int(mode[15][2])) == lr_ms and mode[15][1] == 0 and mode[15][3] == 0
    assert tuple(int(x) for x in block[15][:4]) == bt and block[15][4] == 0
    assert block[15][5] == frames * channels * ngr == sum(bt)
    if "vbr" in name or "abr" in name:
        assert rates >= 3
    if name == "vbr2_js_44k":
        assert mode[15][0] > 0 and mode[15][2] > 0 and all(x > 0 for x in block[15][:4])
    if name in LSF:
        assert ngr == 1 and block[15][5] == frames * channels
