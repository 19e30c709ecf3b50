"""The host twins of the energy VAD (cn_frame_energy_host / cn_vad_decide_host) against the model (tests/vad_model.py): num bit for
bit, e within two 1-ulp logarithms, thr within the bound of any summation order, dec exactly; the refusals; the ABI.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import segments_cases as S
import vad_model as M
from cassnat_asr_public_amd import abi, build, hip

NAMES = ["cn_op_frame_energy", "cn_frame_energy_host", "cn_op_vad_decide", "cn_vad_decide_host"]


def run_host(call, cfg, remove_dc):
    N, shift, channels, channel = cfg
    num, e = np.full(call["size"], M.SENTINEL_NUM, np.int64), np.full(call["size"], M.SENTINEL_E, np.float64)
    hip.frame_energy_host(call["staged"], call["off"], call["samples"], call["out_off"], N, shift, channels, channel, remove_dc,
                          call["max_frames"], num, e, staged_bytes=call["staged_bytes"])
    return num, e


def check_energy(call, cfg, remove_dc, num, e):
    N, shift, channels, channel = cfg
    want = M.frame_energy_fast(call["staged"], call["off"], call["samples"], call["out_off"], N, shift, channels, channel, remove_dc,
                               call["max_frames"], call["staged_bytes"])
    assert want, "a call without frames checks nothing"
    for at, (m, v) in want.items():
        assert int(num[at]) == m, (cfg, at)
        assert abs(e[at] - v) <= M.e_bound(v), (cfg, at, e[at], v)
    rest = np.ones(call["size"], bool)
    rest[list(want)] = False
    assert (num[rest] == M.SENTINEL_NUM).all() and (e[rest] == M.SENTINEL_E).all(), cfg
    assert rest[:M.MARGIN].all() and rest[-M.MARGIN:].all()
    return len(want)


@pytest.mark.parametrize("remove_dc", [True, False])
@pytest.mark.parametrize("cfg", M.ENERGY_CONFIGS)
def test_frame_energy_host_against_the_model(cfg, remove_dc):
    calls = M.energy_calls(cfg)
    assert [len(c["off"]) for c in calls] == [1, 3, 33, 2]
    for call in calls:
        check_energy(call, cfg, remove_dc, *run_host(call, cfg, remove_dc))
    cut = calls[-1]  # staged_bytes lies inside the last row and inside a sample frame: 40 frames and three samples of it exist
    got = M.frame_energy_fast(cut["staged"], cut["off"][-1:], cut["samples"][-1:], [0], *cfg, remove_dc, cut["max_frames"], cut["staged_bytes"])
    N, shift = cfg[:2]
    assert len(got) == M.num_frames((40 - 1) * shift + N + 3, N, shift) < 65


def test_the_fast_model_is_the_integer_model():
    cfg = (200, 80, 1, 0)
    call = M.energy_calls(cfg)[0]
    args = (call["staged"], call["off"], call["samples"], call["out_off"], *cfg, True, call["max_frames"])
    assert M.frame_energy(*args) == M.frame_energy_fast(*args)


def test_the_extreme_rows_through_the_twin():
    for N in (2, 400, 2048):
        for name, x, with_dc, without in M.extreme_rows(N):
            staged = np.frombuffer(x.astype("<i2").tobytes(), np.uint8).copy()
            for remove_dc, want in ((True, with_dc), (False, without)):
                num, e = np.zeros(1, np.int64), np.zeros(1, np.float64)
                hip.frame_energy_host(staged, np.zeros(1, np.int32), np.array([N], np.int32), np.zeros(1, np.int32), N, 1, 1, 0, remove_dc, 1, num, e)
                assert int(num[0]) == want and abs(e[0] - M.log_energy(want, N, remove_dc)) <= M.e_bound(e[0]), (name, N)


def decide_host(es, thr0, scale, context, proportion):
    """Several recordings in one call -> [(thr, dec)]"""
    lens = np.array([len(e) for e in es], np.int32)
    offs = np.concatenate([[2], 2 + np.cumsum(lens[:-1] + 3)]).astype(np.int32)  # (gaps between the recordings)
    total = int(offs[-1] + lens[-1]) + 2
    e = np.full(total, 1e9)
    for o, x in zip(offs, es):
        e[o:o + len(x)] = x
    thr, dec = np.full(len(es), -1.0), np.full(total, 9, np.uint8)
    hip.vad_decide_host(e, offs, lens, thr0, scale, context, proportion, thr, dec)
    mask = np.ones(total, bool)
    for o, n in zip(offs, lens):
        mask[o:o + n] = False
    assert (dec[mask] == 9).all()
    return [(float(thr[i]), dec[o:o + n].tolist()) for i, (o, n) in enumerate(zip(offs, lens))]


def test_decide_host_on_the_crafted_arrays():
    for name, e, thr0, scale, context, proportion in M.decide_cases():
        (thr, dec), = decide_host([e], thr0, scale, context, proportion)
        want_thr, want = M.decide(e, thr0, scale, context, proportion)
        assert thr == want_thr and dec == want, name  # (thr is exact in these cases)
    # three recordings in one call, one of them empty
    es = [M.crafted_e(65), np.zeros(0), M.crafted_e(1000)]
    got = decide_host(es, 5.0, 0.0, 2, 0.5)
    assert got == [M.decide(e, 5.0, 0.0, 2, 0.5) for e in es] and got[1] == (5.0, [])
    got = decide_host([M.crafted_e(64), np.zeros(0), np.array([4.0, 8.0])], 3.0, 0.5, 0, 0.5)
    assert got[1] == (3.0, []) and got[2] == (6.0, [0, 1]) and got[0] == M.decide(M.crafted_e(64), 3.0, 0.5, 0, 0.5)


def audio_energies():
    x = S.recording()
    staged = np.frombuffer(x.tobytes(), np.uint8).copy()
    T = M.num_frames(len(x), 400, 160)
    num, e = np.zeros(T, np.int64), np.zeros(T, np.float64)
    hip.frame_energy_host(staged, np.zeros(1, np.int32), np.array([len(x)], np.int32), np.zeros(1, np.int32), 400, 160, 1, 0, True, T, num, e)
    return e


@pytest.mark.parametrize("context, proportion", [(0, 0.6), (2, 0.6), (5, 0.3)])
def test_decide_host_on_the_audio_case(context, proportion):
    e = audio_energies()
    want_thr, want = M.decide(e, 5.0, 0.5, context, proportion)
    assert M.margin(e, want_thr) > 1e-6, "a frame lies too near the threshold: change the signal, not the bound"
    (thr, dec), = decide_host([e], 5.0, 0.5, context, proportion)
    assert abs(thr - want_thr) <= M.thr_bound(e, 0.5)
    assert dec == want
    if context == 0:
        from cassnat_asr_public_amd.utils import vad

        assert len(vad.runs_of(dec)) == 3


def test_refusals_leave_the_outputs_alone():
    num, e = np.full(8, M.SENTINEL_NUM, np.int64), np.full(8, M.SENTINEL_E, np.float64)
    staged, one = np.zeros(64, np.uint8), np.zeros(1, np.int32)
    n = np.array([16], np.int32)
    L = hip.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = dict(rows=1, N=4, shift=2, channels=1, channel=0, max_frames=4)
    for bad, word in ((dict(rows=0), "rows"), (dict(N=0), "frame length"), (dict(N=2049), "frame length"), (dict(shift=0), "shift"),
                      (dict(channels=0), "channels"), (dict(channels=9), "channels"), (dict(channel=1), "channel"), (dict(channel=-1), "channel")):
        a = dict(good, **bad)
        rc = L.cn_frame_energy_host(p(staged), 64, p(one), p(n), p(one), a["rows"], a["N"], a["shift"], a["channels"], a["channel"], 1,
                                    a["max_frames"], p(num), p(e))
        assert rc == -1 and word in L.cn_last_error().decode(), bad
    assert L.cn_frame_energy_host(None, 64, p(one), p(n), p(one), 1, 4, 2, 1, 0, 1, 4, p(num), p(e)) == -1 and "null" in L.cn_last_error().decode()
    assert (num == M.SENTINEL_NUM).all() and (e == M.SENTINEL_E).all()
    thr, dec, ee = np.zeros(1), np.full(8, 9, np.uint8), np.zeros(8)
    for recs, context in ((0, 0), (1, 65), (1, -1)):
        assert L.cn_vad_decide_host(p(ee), p(one), p(n), recs, 5.0, 0.5, context, 0.6, p(thr), p(dec)) == -1
    assert L.cn_vad_decide_host(p(ee), p(one), p(n), 1, 5.0, 0.5, 0, 0.6, None, p(dec)) == -1
    assert (dec == 9).all()


def test_the_abi():
    assert sorted(abi.VAD_FUNCTIONS) == sorted(NAMES) and abi.VAD_CONSTANTS["CN_VAD_PARTS"] == hip.VAD_PARTS == 64
    assert not set(NAMES) & set(abi.FUNCTIONS)
    assert abi.VAD_FUNCTIONS["cn_op_vad_decide"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double] + [C.c_void_p] * 3)
    assert len(abi.VAD_FUNCTIONS["cn_op_frame_energy"][1]) == 15 and len(abi.VAD_FUNCTIONS["cn_frame_energy_host"][1]) == 14
    for flavour, path in ((None, build.LIB), ("f16", build.LIB_F16)):
        L = hip.lib(flavour)
        for name in NAMES:
            assert getattr(L, name).argtypes == abi.VAD_FUNCTIONS[name][1]
    assert "vad.hip" in build.SOURCES
