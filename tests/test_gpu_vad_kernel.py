"""The energy VAD's kernels against their serial host twins (which tests/test_vad_host.py holds to the model): cn_op_frame_energy - num
bit for bit, sentinels on both sides of both outputs, e within two 1-ulp logarithms - over the case lists of tests/vad_model.py, and
cn_op_vad_decide - dec exactly, thr within the bound of any summation order - on the crafted arrays, the audio case and a recording of
300000 frames.  Both libraries."""
import ctypes as C

import numpy as np
import pytest
import torch

import vad_model as M
from test_vad_host import audio_energies, run_host
from cassnat_asr_public_amd import hip

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_device(call, cfg, remove_dc, flavour=None):
    N, shift, channels, channel = cfg
    num, e = dev(np.full(call["size"], M.SENTINEL_NUM, np.int64)), dev(np.full(call["size"], M.SENTINEL_E, np.float64))
    hip.frame_energy(dev(call["staged"]), call["staged_bytes"], dev(call["off"]), dev(call["samples"]), dev(call["out_off"]), len(call["off"]),
                     N, shift, channels, channel, remove_dc, call["max_frames"], num, e, flavour=flavour)
    torch.cuda.synchronize()
    return num.cpu().numpy(), e.cpu().numpy()


@pytest.mark.parametrize("remove_dc", [True, False])
@pytest.mark.parametrize("cfg", M.ENERGY_CONFIGS)
def test_frame_energy_against_the_host_twin(cfg, remove_dc):
    for call in M.energy_calls(cfg):
        want_num, want_e = run_host(call, cfg, remove_dc)
        num, e = run_device(call, cfg, remove_dc)
        np.testing.assert_array_equal(num, want_num)  # (sentinels included: nothing but the frames that exist is written)
        written = want_num != M.SENTINEL_NUM
        assert written.any() and not written[:M.MARGIN].any() and not written[-M.MARGIN:].any()
        assert (e[~written] == M.SENTINEL_E).all()
        assert (np.abs(e[written] - want_e[written]) <= 4 * 2.0 ** -52 * np.maximum(1.0, np.abs(want_e[written]))).all()


def test_frame_energy_in_the_second_library():
    cfg = (1200, 480, 2, 1)
    call = M.energy_calls(cfg)[1]
    want_num, _ = run_host(call, cfg, True)
    num, _ = run_device(call, cfg, True, flavour="f16")
    np.testing.assert_array_equal(num, want_num)


def test_refusals_leave_the_outputs_alone():
    num, e = dev(np.full(8, M.SENTINEL_NUM, np.int64)), dev(np.full(8, M.SENTINEL_E, np.float64))
    staged, one, n = dev(np.zeros(64, np.uint8)), dev(np.zeros(1, np.int32)), dev(np.array([16], np.int32))
    good = dict(rows=1, N=4, shift=2, channels=1, channel=0, max_frames=4)
    for bad in (dict(rows=0), dict(N=0), dict(N=2049), dict(shift=0), dict(channels=0), dict(channels=9), dict(channel=1), dict(channel=-1)):
        a = dict(good, **bad)
        with pytest.raises(hip.HipError, match="cn_op_frame_energy"):
            hip.frame_energy(staged, 64, one, n, one, a["rows"], a["N"], a["shift"], a["channels"], a["channel"], True, a["max_frames"], num, e)
    L = hip.lib()
    assert L.cn_op_frame_energy(None, 64, hip._ptr(one), hip._ptr(n), hip._ptr(one), 1, 4, 2, 1, 0, 1, 4, hip._ptr(num), hip._ptr(e), None) == -1
    dec, thr = dev(np.full(8, 9, np.uint8)), dev(np.zeros(1 + hip.VAD_PARTS))
    for recs, context in ((0, 0), (1, 65), (1, -1)):
        with pytest.raises(hip.HipError, match="cn_op_vad_decide"):
            hip.vad_decide(e, one, n, recs, 5.0, 0.5, context, 0.6, thr.repeat(max(1, recs)), dec)
    torch.cuda.synchronize()
    assert (num.cpu().numpy() == M.SENTINEL_NUM).all() and (e.cpu().numpy() == M.SENTINEL_E).all() and (dec.cpu().numpy() == 9).all()


def decide_both(es, thr0, scale, context, proportion, flavour=None):
    """Several recordings in one call on the device and through the twin -> [(thr, dec)] of each, and the untouched gaps checked."""
    lens = np.array([len(e) for e in es], np.int32)
    offs = np.concatenate([[2], 2 + np.cumsum(lens[:-1] + 3)]).astype(np.int32)
    total = int(offs[-1] + lens[-1]) + 2
    e = np.full(total, 1e9)
    for o, x in zip(offs, es):
        e[o:o + len(x)] = x
    thr_h, dec_h = np.full(len(es), -1.0), np.full(total, 9, np.uint8)
    hip.vad_decide_host(e, offs, lens, thr0, scale, context, proportion, thr_h, dec_h)
    thr_d, dec_d = dev(np.full(len(es) * (1 + hip.VAD_PARTS), -1.0)), dev(np.full(total, 9, np.uint8))
    hip.vad_decide(dev(e), dev(offs), dev(lens), len(es), thr0, scale, context, proportion, thr_d, dec_d, flavour=flavour)
    torch.cuda.synchronize()
    return thr_h, dec_h, thr_d.cpu().numpy()[:len(es)], dec_d.cpu().numpy()


def test_decide_on_the_crafted_arrays():
    cases = M.decide_cases()
    for key in sorted({c[2:] for c in cases}):  # (the recordings that share the options go in one call, with an empty one among them)
        es = [c[1] for c in cases if c[2:] == key]
        es.insert(1, np.zeros(0))
        thr_h, dec_h, thr_d, dec_d = decide_both(es, *key)
        np.testing.assert_array_equal(thr_d, thr_h)  # (thr is exact in these cases)
        np.testing.assert_array_equal(dec_d, dec_h)


@pytest.mark.parametrize("flavour", [None, "f16"])
def test_decide_on_the_audio_case_and_a_long_recording(flavour):
    e = audio_energies()
    want_thr = M.threshold(e, 5.0, 0.5)  # (the model's: an exactly rounded sum)
    assert M.margin(e, want_thr) > 1e-6, "a frame lies too near the threshold: change the signal, not the bound"
    for context, proportion in ((0, 0.6), (2, 0.6)):
        thr_h, dec_h, thr_d, dec_d = decide_both([e], 5.0, 0.5, context, proportion, flavour)
        assert abs(thr_d[0] - want_thr) <= M.thr_bound(e, 0.5)
        np.testing.assert_array_equal(dec_d, dec_h)
        assert dec_d[2:2 + len(e)].tolist() == M.decide(e, 5.0, 0.5, context, proportion)[1]
    # 300000 frames of quarters: every partial sum is exact, so the two-level mean equals the serial one bit for bit
    big = np.random.RandomState(5).randint(0, 81, 300000) / 4.0
    thr_h, dec_h, thr_d, dec_d = decide_both([big, M.crafted_e(65)], 1.0, 0.5, 3, 0.5, flavour)
    np.testing.assert_array_equal(thr_d, thr_h)
    np.testing.assert_array_equal(dec_d, dec_h)
    assert 0 < dec_d.sum() < dec_d.size
