"""The model of the energy VAD (tests/vad_model.py) against values worked out by hand, its segmentation - and utils/vad.py's - against
a brute-force restatement on every decision string of up to 12 frames, and five planted mistakes, each caught by the case lists.
No GPU, no library."""
import itertools
import math

import numpy as np
import pytest

import vad_model as M
from cassnat_asr_public_amd.utils import vad

LOG_FLOOR = -15.942385152878742  # log(2^-23) = -23 ln 2


@pytest.mark.parametrize("N", [1, 2, 400, 2048])
def test_the_extreme_frames_by_hand(N):
    assert math.log(M.FLOOR) == LOG_FLOOR
    for name, x, with_dc, without in M.extreme_rows(N):
        assert M.frame_num(x, N, True) == with_dc and M.frame_num(x, N, False) == without, name
        assert M.log_energy(without, N, False) == math.log(float(without))
    # a constant frame: num = 0 with DC removal, the clamp
    assert M.log_energy(0, N, True) == LOG_FLOOR and M.log_energy(0, N, False) == LOG_FLOOR
    # the all -32768 frame holds the largest S2 = N 2^30
    assert M.frame_num(np.full(N, -32768, np.int16), N, False) == N << 30
    if N % 2 == 0:  # alternating 32767 / -32768: deviations of +-32767.5 from the mean -0.5, so num / N^2 = 32767.5^2
        num = M.frame_num(np.tile(np.array([32767, -32768], np.int16), N // 2), N, True)
        assert num * 4 == N * N * 65535 * 65535 and num < 2 ** 52


def test_frames_and_rows():
    assert [M.num_frames(n, 400, 160) for n in (0, 399, 400, 559, 560, 720)] == [0, 0, 1, 1, 2, 3]
    assert M.row_samples(16, 100, 2, 16 + 4 * 50 + 3) == 50 and M.row_samples(7, 100, 1, 1000) == 0 and M.row_samples(-16, 5, 1, 100) == 0
    x = np.arange(-6, 6, dtype="<i2")
    staged = np.frombuffer(x.tobytes(), np.uint8)
    got = M.frame_energy(staged, [0], [6], [3], 2, 2, 2, 1, False, 10)  # channel 1 of 6 stereo sample frames: -5, -3, -1, 1, 3, 5
    assert {k: v[0] for k, v in got.items()} == {3: 25 + 9, 4: 1 + 1, 5: 9 + 25}
    assert list(M.frame_energy(staged, [0], [6], [3], 2, 2, 2, 1, False, 2)) == [3, 4]


def brute_segments(dec, e, min_silence, min_speech, pad, max_segment):
    """The five rules on labelled frames instead of run lists."""
    T = len(dec)
    m = list(dec)
    ones = [t for t in range(T) if dec[t]]
    for a, b in zip(ones, ones[1:]):  # 1. + 2.: a gap of zeros between two ones that is shorter than min_silence is filled
        if 0 < b - a - 1 < min_silence:
            for t in range(a + 1, b):
                m[t] = 1
    starts = [t for t in range(T) if m[t] and (t == 0 or not m[t - 1])]
    stops = [t + 1 for t in range(T) if m[t] and (t == T - 1 or not m[t + 1])]
    runs = [(a, b) for a, b in zip(starts, stops) if b - a >= min_speech]  # 3.
    out = []
    for i, (a, b) in enumerate(runs):  # 4.
        lo, hi = max(0, a - pad), min(T, b + pad)
        if i > 0 and min(T, runs[i - 1][1] + pad) > lo:
            lo = (runs[i - 1][1] + a) // 2
        if i + 1 < len(runs) and hi > max(0, runs[i + 1][0] - pad):
            hi = (b + runs[i + 1][0]) // 2
        out.append((lo, hi))
    cut = []
    for a, b in out:  # 5.
        while b - a > max_segment:
            c = sorted(range(a + max_segment // 2, a + max_segment), key=lambda t: (e[t], t))[0]
            cut.append((a, c))
            a = c
        cut.append((a, b))
    return cut


@pytest.mark.parametrize("params", [(2, 2, 1, 4), (3, 3, 2, 5), (1, 1, 0, 2), (4, 1, 3, 6)])
def test_segmentation_against_brute_force_on_every_short_string(params):
    for T in range(0, 13):
        e = [float((5 * t + 3) % 4) for t in range(T)]  # (ties inside every window of two or more frames)
        for dec in itertools.product((0, 1), repeat=T):
            want = brute_segments(dec, e, *params)
            assert M.segment(dec, e, *params) == want, (dec, params)
            assert vad.segment(dec, e, *params) == want, (dec, params)


def test_the_hand_made_cases():
    for name, dec, e, *rest in M.segment_cases():
        params, want = rest[:4], rest[4]
        assert M.segment(dec, e, *params) == want, name
        assert vad.segment(dec, e, *params) == want, name
    assert vad.runs_of([0, 1, 1, 0, 1]) == [(1, 3), (4, 5)]
    with pytest.raises(ValueError, match="at least 2"):
        vad.segment([1, 1], [0.0, 0.0], 1, 1, 0, 1)


def test_the_crafted_decisions_by_hand():
    e = M.crafted_e(65)
    thr, dec = M.decide(e, 5.0, 0.0, 0, 1.0)
    assert thr == 5.0 and dec[:4] == [1, 1, 0, 0]  # e[2] == thr says non-speech
    assert M.decide(e, 5.0, 0.0, 2, 0.5)[1][1] == 1  # the exact tie 2 >= 4 * 0.5 says speech
    assert M.decide(e, 5.0, 0.0, 2, 0.5)[1][0] == 1  # the window of t = 0 is clipped to three frames: 2 >= 1.5
    assert M.decide(e, 5.0, 0.0, 64, 0.0)[1] == [1] * 65
    assert M.decide([4.0, 8.0], 3.0, 0.5, 0, 0.5) == (6.0, [0, 1]) and M.decide([6.0, 6.0], 3.0, 0.5, 0, 0.5) == (6.0, [0, 0])
    assert M.decide([], 3.0, 0.5, 2, 0.5) == (3.0, [])


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_every_planted_mistake_is_caught(mistake):
    caught = []
    for name, e, thr0, scale, context, proportion in M.decide_cases():
        if M.decide(e, thr0, scale, context, proportion, mistake=mistake) != M.decide(e, thr0, scale, context, proportion):
            caught.append(name)
    for name, dec, e, *rest in M.segment_cases():
        if M.segment(dec, e, *rest[:4], mistake=mistake) != rest[4]:
            caught.append(name)
    assert caught, mistake


def test_the_option_file(tmp_path):
    conf = tmp_path / "vad.conf"
    conf.write_text("# energy VAD\n--vad-energy-threshold=5.5\n--vad-frames-context=2  # both sides\n\n")
    assert vad.parse_vad_conf(str(conf)) == {"thr0": 5.5, "mean_scale": 0.5, "context": 2, "proportion": 0.6}
    assert vad.parse_vad_conf("") == {"thr0": 5.0, "mean_scale": 0.5, "context": 0, "proportion": 0.6}
    conf.write_text("--vad-energy-threshold=5.5\n--dither=0\n")
    with pytest.raises(ValueError, match="--dither"):
        vad.parse_vad_conf(str(conf))
    conf.write_text("--vad-frames-context=65\n")
    with pytest.raises(ValueError, match="65"):
        vad.parse_vad_conf(str(conf))
    assert [vad.frames_of_seconds(s, 0.01) for s in (0.3, 0.2, 0.1, 30)] == [30, 20, 10, 3000]
