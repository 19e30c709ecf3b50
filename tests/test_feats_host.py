"""The feature-archive writer, the parts that need no GPU: the companion header and its binding, and the host twins
cn_compress_feats_host / cn_feats_stats_host of both libraries against the model (tests/feats_model.py) over the whole case list
(tests/feats_cases.py) - every payload byte, every status word, and the sentinel bytes in front of, between and behind the payloads."""
import math

import numpy as np
import pytest

import feats_cases
import feats_model as M
from cassnat_asr_public_amd import abi, hip
from cassnat_asr_public_amd.data import kaldi_io

NEW = ["cn_compress_feats_bytes", "cn_op_compress_feats", "cn_compress_feats_host", "cn_op_feats_stats", "cn_feats_stats_host"]
SENTINEL = 0xA5
FRONT = 64  # sentinel bytes in front of the first payload (a multiple of 16)


def run_host(case, flavour):
    """-> (out with sentinels, offsets, status, the model's out and status)."""
    feats, lens = case["feats"], case["lens"]
    rows, tmax, F = feats.shape
    offs, end = M.layout(lens, F, tmax)
    offs = (offs + FRONT).astype(np.int32)
    out = np.full(FRONT + end + 48, SENTINEL, np.uint8)
    want = out.copy()
    status = np.full(rows, -9, np.int32)
    hip.compress_feats_host(feats, lens, offs, out, status, flavour=flavour)
    return out, offs, status, want, M.compress_batch(feats, lens, offs, want)


def test_entry_points_are_declared_in_the_new_header_only_and_exported_by_both_libraries():
    assert sorted(abi.FEATS_FUNCTIONS) == sorted(NEW)
    older = (set(abi.FUNCTIONS) | set(abi.EXTRA_FUNCTIONS) | set(abi.PROJ_FUNCTIONS) | set(abi.AST_NGRAM_FUNCTIONS) | set(abi.NAT_NGRAM_FUNCTIONS)
             | set(abi.CTC_TIMES_FUNCTIONS) | set(abi.SCORE_FUNCTIONS) | set(abi.CTC_BIAS_FUNCTIONS) | set(abi.AST_BIAS_FUNCTIONS))
    assert not set(NEW) & older
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        assert all(hasattr(L, n) for n in NEW)


def test_payload_bytes():
    for T in (0, 1, 8, 9, 1031):
        for F in (1, 80, 83):
            assert hip.compress_feats_bytes(T, F) == M.payload_bytes(T, F) == (16 + 8 * F + T * F if T > 8 else 16 + 2 * T * F)
    assert hip.compress_feats_bytes(-1, 80) == 0 and hip.compress_feats_bytes(5, 0) == 0
    offs, sizes, total = hip.compress_feats_layout([9, 3, 0, 2000], 80, tmax=100)
    assert offs.tolist() == M.layout([9, 3, 0, 2000], 80, 100)[0].tolist() and total == M.layout([9, 3, 0, 2000], 80, 100)[1]
    assert all(o % 16 == 0 for o in offs.tolist()) and sizes.tolist() == [M.payload_bytes(t, 80) for t in (9, 3, 0, 100)]


@pytest.mark.parametrize("flavour", [None, "f16"])
def test_the_host_twin_equals_the_model_in_every_byte(flavour):
    for case in feats_cases.CASES:
        out, offs, status, want, want_status = run_host(case, flavour)
        assert status.tolist() == want_status.tolist(), case["name"]
        bad = np.nonzero(out != want)[0]
        assert bad.size == 0, (case["name"], int(bad[0]), offs.tolist()[:4])
        # (the model wrote nothing outside the payloads either: the sentinels in front, in the gaps and behind are part of `want`)
        assert (want[:FRONT] == SENTINEL).all() and (want[-48:] == SENTINEL).all()


def test_the_gaps_between_payloads_are_really_there():
    case = next(c for c in feats_cases.CASES if c["name"] == "ragged_33")
    out, offs, status, _, _ = run_host(case, None)
    F, tmax = case["feats"].shape[2], case["feats"].shape[1]
    ends = [int(o) + M.payload_bytes(min(int(n), tmax), F) for o, n in zip(offs, case["lens"])]
    gaps = [(e, int(o)) for e, o in zip(ends[:-1], offs[1:]) if o > e]
    assert gaps and all((out[a:b] == SENTINEL).all() for a, b in gaps)


def stored_values(case, r, out, offs):
    x = feats_cases.valid(case, r)
    T, F = x.shape
    kind = "CM" if T > 8 else "CM2"
    return kaldi_io.decompress(kind, T, F, out[int(offs[r]):int(offs[r]) + M.payload_bytes(T, F)])


@pytest.mark.parametrize("flavour", [None, "f16"])
def test_the_stats_twin_lies_within_the_bound_and_repeats(flavour):
    for case in feats_cases.CASES:
        feats, lens = case["feats"], case["lens"]
        rows, tmax, F = feats.shape
        if F > 83 or tmax > 300:
            continue
        out, offs, status, _, _ = run_host(case, flavour)
        for payload in (out, None):
            got = hip.feats_stats_host(feats, lens, payload=payload, out_off=None if payload is None else offs, status=status, flavour=flavour)
            again = hip.feats_stats_host(feats, lens, payload=payload, out_off=None if payload is None else offs, status=status, flavour=flavour)
            assert got.tobytes() == again.tobytes()
            for r in range(rows):
                if status[r] != 0:
                    assert not got[r].any(), (case["name"], r)
                    continue
                v = stored_values(case, r, out, offs) if payload is not None else feats_cases.valid(case, r)
                assert (np.abs(got[r] - M.exact_stats(v)) <= M.stats_bound(v)).all(), (case["name"], r, payload is None)


def test_refusals():
    feats = np.zeros((1, 4, 3), np.float32)
    lens, offs, status, out = np.array([4], np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(64, np.uint8)
    L = hip.lib()
    p = lambda a: a.ctypes.data_as(hip.C.c_void_p)
    assert L.cn_compress_feats_host(None, p(lens), p(offs), 1, 4, 3, p(out), 64, p(status)) == -1
    assert L.cn_compress_feats_host(p(feats), p(lens), p(offs), 0, 4, 3, p(out), 64, p(status)) == -1
    assert L.cn_compress_feats_host(p(feats), p(lens), p(offs), 1, 4, 0, p(out), 64, p(status)) == -1
    assert b"cn_compress_feats_host" in L.cn_last_error()
    # a payload that would leave the buffer, or that starts off a multiple of 16: status 3, nothing written
    out[:] = SENTINEL
    assert L.cn_compress_feats_host(p(feats), p(lens), p(offs), 1, 4, 3, p(out), 16 + 2 * 4 * 3 - 1, p(status)) == 0
    assert status[0] == 3 and (out == SENTINEL).all()
    offs[0] = 8
    assert L.cn_compress_feats_host(p(feats), p(lens), p(offs), 1, 4, 3, p(out), 64, p(status)) == 0
    assert status[0] == 3 and (out == SENTINEL).all()
    assert math.isfinite(hip.feats_stats_host(feats, lens).sum())
