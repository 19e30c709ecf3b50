"""The compression and stats kernels (cn_op_compress_feats, cn_op_feats_stats) against the host twins and the model
(tests/feats_model.py): every payload byte, every status word and the sentinels in front of, between and behind the payloads over the
whole case list, in both libraries, with NO tolerance; the stats within the bound of any summation order of math.fsum over what the
existing reader decompresses from the kernel's own bytes, and bit-identical across two launches."""
import numpy as np
import pytest
import torch

import feats_cases
import feats_model as M
from cassnat_asr_public_amd import hip
from test_feats_host import FRONT, SENTINEL, run_host, stored_values

pytestmark = pytest.mark.gpu


def run_device(case, flavour):
    feats, lens = case["feats"], case["lens"]
    rows, tmax, F = feats.shape
    offs, end = M.layout(lens, F, tmax)
    offs = (offs + FRONT).astype(np.int32)
    d_feats, d_lens, d_offs = torch.from_numpy(feats).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(offs).cuda()
    d_out = torch.full((FRONT + end + 48,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_status = torch.full((rows,), -9, dtype=torch.int32, device="cuda")
    hip.compress_feats(d_feats, d_lens, d_offs, d_out, d_status, flavour=flavour)
    torch.cuda.synchronize()
    return d_feats, d_lens, d_offs, d_out, d_status


@pytest.mark.parametrize("flavour", [None, "f16"])
def test_the_kernel_equals_the_host_twin_byte_for_byte(flavour):
    for case in feats_cases.CASES:
        out, offs, status, want, want_status = run_host(case, flavour)
        _, _, _, d_out, d_status = run_device(case, flavour)
        got, got_status = d_out.cpu().numpy(), d_status.cpu().numpy()
        assert got_status.tolist() == status.tolist() == want_status.tolist(), case["name"]
        bad = np.nonzero(got != out)[0]
        assert bad.size == 0, (case["name"], int(bad[0]), int(bad.size), offs.tolist()[:4])
        assert (got == want).all(), case["name"]  # (the model, sentinels included)


@pytest.mark.parametrize("flavour", [None, "f16"])
def test_the_stats_kernel_lies_within_the_bound_and_repeats_bit_for_bit(flavour):
    for case in feats_cases.CASES:
        rows, tmax, F = case["feats"].shape
        if tmax > 300 and F > 17:  # (the exact sums in Python take their time; the long and the wide shapes are each covered)
            continue
        d_feats, d_lens, d_offs, d_out, d_status = run_device(case, flavour)
        out, status = d_out.cpu().numpy(), d_status.cpu().numpy()
        for compressed in (True, False):
            runs = []
            for _ in range(2):
                d_stats = torch.full((rows, 2, F), float("nan"), dtype=torch.float64, device="cuda")
                hip.feats_stats(d_feats, d_lens, d_stats, payload=d_out if compressed else None, out_off=d_offs if compressed else None,
                                status=d_status, flavour=flavour)
                torch.cuda.synchronize()
                runs.append(d_stats.cpu().numpy())
            assert runs[0].tobytes() == runs[1].tobytes(), case["name"]
            twin = hip.feats_stats_host(case["feats"], case["lens"], payload=out if compressed else None,
                                        out_off=d_offs.cpu().numpy() if compressed else None, status=status, flavour=flavour)
            assert runs[0].tobytes() == twin.tobytes(), case["name"]  # (the twin adds in the kernel's order)
            for r in range(rows):
                if status[r] != 0:
                    assert not runs[0][r].any(), (case["name"], r)
                    continue
                v = stored_values(case, r, out, d_offs.cpu().numpy()) if compressed else feats_cases.valid(case, r)
                assert (np.abs(runs[0][r] - M.exact_stats(v)) <= M.stats_bound(v)).all(), (case["name"], r, compressed)


def test_refusals_launch_nothing():
    feats = torch.zeros((1, 4, 3), device="cuda")
    lens, offs = torch.tensor([4], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    out, status = torch.full((80,), SENTINEL, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipError):
        hip.compress_feats(feats, lens, offs, out[1:], status)  # (not on a 16-byte boundary)
    hip.compress_feats(feats, lens, offs, out[:16 + 2 * 4 * 3 - 1], status)  # (a payload that would leave the buffer)
    torch.cuda.synchronize()
    assert int(status[0]) == 3 and bool((out == SENTINEL).all())
