"""The model of the matrix compression (tests/feats_model.py) against bytes worked out by hand, against the existing
reader (kaldi_io.decompress) under a cap that follows from the format, and against five deliberate mistakes, each of which the case
list (tests/feats_cases.py) must catch; the stats model against math.fsum."""
import struct

import numpy as np
import pytest

import feats_cases
import feats_model as M
from cassnat_asr_public_amd.data import kaldi_io

CASES = feats_cases.CASES


def good_utterances():
    for case in CASES:
        for r in range(case["feats"].shape[0]):
            x = feats_cases.valid(case, r)
            if x.shape[0] >= 1 and np.isfinite(x).all():
                yield case["name"], r, x


def test_a_three_by_two_matrix_by_hand():
    # min 0, range 8; 4 / 8 * 65535 = 32767.5, and + 0.499 leaves 32767 where + 0.5 would give 32768
    status, token, payload = M.compress(np.array([[0, 1], [2, 3], [4, 8]], np.float32))
    assert (status, token) == (0, b"CM2 ")
    assert payload == struct.pack("<ffii", 0.0, 8.0, 3, 2) + struct.pack("<6H", 0, 8192, 16384, 24576, 32767, 65535)


def test_a_nine_by_one_matrix_by_hand():
    # min 0, range 8, q = 2: the sorted values at 0, 2, 6, 8 are 0, 2, 6, 8 with the codes 0, 16384, 49151 (0.75 * 65535 + 0.499 =
    # 49151.749) and 65535.  P25 = 16384 * 8 / 65535 = 2.00003 lies just above 2, so 2 is coded in the first segment as 64;
    # P75 = 49151 * 8 / 65535 = 5.99997 lies just below 6, so 6 opens the third segment as 192.  In the middle segment of width 3.99994
    # the values 3, 4, 5 sit at 0.99997, 1.99997, 2.99997: 32, 64, 96 codes of 128; 7 sits at 1.00003 of 2.00003: 31.5005 + 0.5 -> 32.
    status, token, payload = M.compress(np.arange(9, dtype=np.float32).reshape(9, 1))
    assert (status, token) == (0, b"CM ")
    want = struct.pack("<ffii", 0.0, 8.0, 9, 1) + struct.pack("<4H", 0, 16384, 49151, 65535) + bytes([0, 32, 64, 96, 128, 160, 192, 224, 255])
    assert payload == want


def test_payload_sizes_and_kinds():
    for T in feats_cases.TS:
        for F in (1, 17, 80):
            status, token, payload = M.compress(np.ones((T, F), np.float32))
            assert status == 0 and token == (b"CM " if T > 8 else b"CM2 ") and len(payload) == M.payload_bytes(T, F)
            assert len(payload) == (16 + 8 * F + T * F if T > 8 else 16 + 2 * T * F)


def test_the_reader_reads_every_case_back_within_the_cap():
    """|decompress(model(x)) - x| <= step / 2 + 2 * range / 65535, step the code width of the segment the value was coded in (at bytes
    64 and 192 the wider neighbour): half a code of the segment, plus the rounding of the four header codes (half a uint16 step each,
    doubled as the margin for cases not drawn).  A cap that follows from the format, not a measurement."""
    n = 0
    for name, r, x in good_utterances():
        status, token, payload = M.compress(x)
        assert status == 0
        kind = token.decode().strip()
        back = kaldi_io.decompress(kind, x.shape[0], x.shape[1], np.frombuffer(payload, np.uint8))
        step, rng = M.steps(x, payload)
        err = np.abs(back.astype(np.float64) - x.astype(np.float64))
        cap = step / 2 + 2 * rng / 65535
        assert (err <= cap).all(), (name, r, float((err / cap).max()))
        n += 1
    assert n > 100


def test_the_cases_hold_what_they_promise():
    by_name = {c["name"]: c for c in CASES}
    # values exactly on P25 and on P75
    case = by_name["on_the_quartiles"]
    for r in (0, 1):
        x = feats_cases.valid(case, r)
        _, _, payload = M.compress(x)
        F = x.shape[1]
        mn, rng = (np.float32(v) for v in struct.unpack("<ff", payload[:8]))
        p = M.quartiles(np.frombuffer(payload[16:16 + 8 * F], "<u2").reshape(F, 4), mn, rng)
        assert all((x[:, c] == p[c, 1]).any() and (x[:, c] == p[c, 2]).any() for c in range(F))
    # the caps 65532 .. 65534 and the forcing
    x = feats_cases.valid(by_name["column_at_the_extremes"], 0)
    _, _, payload = M.compress(x)
    h = np.frombuffer(payload[16:16 + 8 * 4], "<u2").reshape(4, 4)
    assert h[1].tolist() == [65532, 65533, 65534, 65535] and h[3].tolist() == [0, 1, 2, 3]
    # both kinds in one batch, NaN padding, clamped and bad lengths, the status words
    assert {M.compress(feats_cases.valid(by_name["ragged_33"], r))[1] for r in range(33)} == {b"CM ", b"CM2 "}
    assert np.isnan(by_name["ragged_33"]["feats"]).any()
    assert (by_name["lens_above_tmax"]["lens"] > by_name["lens_above_tmax"]["feats"].shape[1]).any()
    c = by_name["not_finite"]
    out = np.zeros(4096, np.uint8)
    assert M.compress_batch(c["feats"], c["lens"], M.layout(c["lens"], 4, 12)[0], out).tolist() == [0, 2, 2, 2, 0]
    c = by_name["no_rows"]
    assert M.compress_batch(c["feats"], c["lens"], M.layout(c["lens"], 4, 10)[0], out).tolist() == [1, 0, 1]
    # T = 10 is where 3 * (T / 4) and 3 * T / 4 part
    assert 3 * (10 // 4) != 3 * 10 // 4


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_a_deliberate_mistake_is_caught_by_the_case_list(mistake):
    caught = [name for name, r, x in good_utterances() if M.compress(x, mistake)[2] != M.compress(x)[2]]
    assert caught, mistake


def test_the_stats_model_lies_within_the_bound_of_any_summation_order():
    n = 0
    for name, r, x in good_utterances():
        if x.shape[1] > 83 or x.shape[0] > 300:
            continue
        status, token, payload = M.compress(x)
        stored = kaldi_io.decompress(token.decode().strip(), x.shape[0], x.shape[1], np.frombuffer(payload, np.uint8))
        for v in (stored, x):  # a compressed payload's values, and the float32 rows
            assert (np.abs(M.stats(v) - M.exact_stats(v)) <= M.stats_bound(v)).all(), (name, r)
        n += 1
    assert n > 50
