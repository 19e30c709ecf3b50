"""Recordings and segment lists shared by the segments / make_segments tests."""
import struct

import numpy as np

import vad_model as M
from test_gpu_wave_reader import int16_wave


def speech(n, seed):
    """n int16 samples of the reader tests' signal (which lasts 1.2 s: a longer stretch is pieces of it in a row)."""
    return np.concatenate([int16_wave(min(19200, n - at), seed + 50 * k) for k, at in enumerate(range(0, n, 19200))])


def write_wave(path, x, rate=16000, channels=1):
    """x: int16, interleaved when channels > 1."""
    data = np.ascontiguousarray(x, dtype="<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, channels, rate, rate * 2 * channels, 2 * channels, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


_rec = {}


def recording():
    """The 80200-sample recording of tests/vad_model.py (16 kHz, mono)."""
    if "x" not in _rec:
        _rec["x"] = M.recording(speech)
    return _rec["x"]


def stereo_441(x):
    """A 44.1 kHz stereo file whose channel 1 holds ``x`` sample for sample (channel 0: other noise) - its VAD at 44.1 kHz differs
    from the mono file's, both legs see the same samples."""
    other = np.random.RandomState(11).randint(-2000, 2000, len(x)).astype("<i2")
    return np.stack([other, x], 1).reshape(-1)
