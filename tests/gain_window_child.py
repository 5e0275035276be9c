"""Child process of tests/test_batch_replaygain_device.py::test_frame_windows_one_analysis, started with LAMEHIP_MID_WINDOW
set: two streams of about 4 s go through a launch that the split pipeline works through in windows of frames; the gain
analysis in front of them ran (gain_ms() > 0), and its windows and gains are the host twin's and the handle's for the whole
streams, whatever the frame windows."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deprecated-lame-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import gain_support as gs
    assert int(os.environ["LAMEHIP_MID_WINDOW"]) > 0
    setting = gs.SETTINGS[0]
    lib = gs.library()
    xs = [gs.signal(setting, 9800, int(4.0 * 44100)), gs.signal(setting, 9801, int(3.7 * 44100), 0.25)]
    want = []
    for x in xs:
        h = gs.open_handle(setting, find_gain=True)
        want.append(gs.handle_stream(h, setting, x)[1])
        h.close()
    enc = gs.open_handle(setting)
    b = gs.make_batch(enc, setting, len(xs), max(x.shape[1] for x in xs))
    b.set_replaygain()
    gs.feed_batch(b, setting, xs)
    b.encode()
    assert b.windows() > 1, "the launch did not run in windows of frames"
    assert b.gain_ms() > 0.0
    for s, x in enumerate(xs):
        pairs, tenths = gs.expected_of_stream(lib, b, enc, setting, s, x)
        assert gs.same_doubles(b.gain_windows(s), pairs), "stream %d: window sums" % s
        assert b.radio_gain(s) == tenths == want[s] != 0, (s, b.radio_gain(s), tenths, want[s])
    assert want[0] != want[1]
    nwin = b.windows()
    b.close()
    enc.close()
    print("gain under frame windows ok: %d windows, gains %s" % (nwin, want), flush=True)


if __name__ == "__main__":
    main()
