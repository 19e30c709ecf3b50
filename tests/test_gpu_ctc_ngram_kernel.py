"""The n-gram search kernel alone (csrc/ctc_beam.hip, through cn_op_ctc_ngram_beam) against cn_ctc_ngram_beam_host, the serial host
loop over the same step functions (itself compared with the float64 model in tests/test_ctc_ngram_host.py), on that file's inputs
and cases: hypotheses and order exact, score_lm bit for bit on the dyadic models, score_ctc / p_blk / p_nblk to 1e-8 (libm's and the
device's log1p / exp may differ in the last bits); 8 elements behind every output stay untouched.  With lm_scale 0 the kernel is
cn_op_ctc_prefix_beam's, the other instantiation of the same body: equal bits."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_ngram_cases as cases
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import _ptr

pytestmark = pytest.mark.gpu


def run_device(case, blank=0):
    lm = cases.lm_of(case.order, case.hash_bits)[0].cuda()
    B, Tp, V = case.logp.shape
    cap = Tp + 1
    o = cases.outputs(B, case.W, cap)
    d = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(o).items()})
    logp, ratio = torch.from_numpy(case.logp).cuda(), torch.from_numpy(case.ratio).cuda()
    top = torch.from_numpy(np.ascontiguousarray(case.top)).cuda() if case.P else None
    rc = hip.lib().cn_op_ctc_ngram_beam(C.byref(lm.desc(lm.device)), _ptr(logp), _ptr(top) if case.P else None, _ptr(ratio), B, Tp, V, case.W,
                                        case.P, case.lp, case.lm_scale, blank, _ptr(d.hyp), cap, _ptr(d.hlen), _ptr(d.sc), _ptr(d.slm),
                                        _ptr(d.pb), _ptr(d.pnb), _ptr(d.nb), hip.current_stream())
    assert rc == 0, hip.lib().cn_last_error()
    torch.cuda.synchronize()
    o = SimpleNamespace(**{k: v.cpu().numpy() for k, v in vars(d).items()})
    assert cases.untouched(o, B, case.W, cap)
    return cases.beams_of(o, B, case.W, cap)


@pytest.mark.parametrize("order", cases.ORDERS)
@pytest.mark.parametrize("beam,pruning", cases.BEAMS)
@pytest.mark.parametrize("Tp", cases.SHAPES)
def test_kernel_is_the_host_search(Tp, beam, pruning, order):
    case = cases.make_case(Tp, beam, pruning, order)
    got = run_device(case)
    cases.same_beams(got, cases.run_host(case))
    assert [e["hyp"] for e in got[2]] == [[]]  # every frame blank: the empty hypothesis, </s> alone
    assert any(e["score_lm"] != 0.0 for seqs in got for e in seqs)


@pytest.mark.parametrize("name", ["repeat", "ties1", "ties3", "collision", "pruning0", "foreign"])
def test_kernel_on_the_crafted_cases(name):
    if name == "repeat":
        case = cases.repeat_case()
    elif name.startswith("ties"):
        case = cases.ties_case(int(name[4:]))
    elif name == "collision":
        case = cases.collision_case()
    elif name == "pruning0":
        case = cases.make_case(12, 2, 0, 2)
    else:  # labels outside [0, V) in the pruned lists make no candidate
        case = cases.make_case(12, 5, 3, 2)
        case.P = 5
        case.top = np.concatenate([np.full(case.top.shape[:2] + (1,), cases.V, np.int32), case.top,
                                   np.full(case.top.shape[:2] + (1,), -3, np.int32)], axis=2)
    cases.same_beams(run_device(case), cases.run_host(case))


@pytest.mark.parametrize("Tp,W,P,lp", [(1, 1, 1, 0.0), (12, 5, 3, 0.25), (40, 32, 8, 0.1), (40, 32, 27, 0.0), (12, 2, 0, 0.3)])
def test_with_lm_scale_zero_it_is_the_prefix_beam_kernel(Tp, W, P, lp):
    """Random log-posteriors (no two equal in a row, so the device's top-k and the list given here are the same)."""
    case = cases.make_case(Tp, W, P, 3, lm_scale=0.0, lp=lp)
    assert all(len(set(row.tolist())) == cases.V for row in case.logp[:2].reshape(-1, cases.V))
    case.logp[2] = case.logp[0][::-1]  # (the prefix beam kernel's top-k has no rule for the all-blank utterance's equal values)
    case.top = cases.topk_lists(case.logp, case.P)
    got = run_device(case)
    B = 3
    logp, ratio = torch.from_numpy(case.logp).cuda(), torch.from_numpy(case.ratio).cuda()
    hyp = torch.zeros(B, W, Tp + 1, dtype=torch.int32, device="cuda")
    hlen, nb = torch.zeros(B, W, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    sc, pb, pnb = (torch.zeros(B, W, dtype=torch.float64, device="cuda") for _ in range(3))
    hip.check(hip.lib().cn_op_ctc_prefix_beam(_ptr(logp), _ptr(ratio), B, Tp, cases.V, W, P, lp, 0, _ptr(hyp), Tp + 1, _ptr(hlen), _ptr(sc),
                                              _ptr(pb), _ptr(pnb), _ptr(nb), hip.current_stream()))
    torch.cuda.synchronize()
    hyp, hlen, sc, pb, pnb, nb = (t.cpu().numpy() for t in (hyp, hlen, sc, pb, pnb, nb))
    for b in range(B):
        assert len(got[b]) == int(nb[b])
        for j, e in enumerate(got[b]):
            assert e["hyp"] == hyp[b, j, :hlen[b, j]].tolist(), (b, j)
            assert e["score_lm"] == 0.0
            # (one kernel body, two instantiations: the same bits)
            assert e["score_ctc"] == sc[b, j] and e["p_blk"] == pb[b, j] and e["p_nblk"] == pnb[b, j]


def test_refusals_leave_the_outputs_alone():
    lm = cases.lm_of(3)[0].cuda()
    case = cases.make_case(12, 5, 3, 3)
    B, Tp, V = case.logp.shape
    o = cases.outputs(B, 5, Tp + 1, pad=0)
    d = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(o).items()})
    logp, ratio, top = (torch.from_numpy(a).cuda() for a in (case.logp, case.ratio, case.top))
    L = hip.lib()
    for W, P, msg in ((0, 3, b"ctc_beam"), (33, 3, b"ctc_beam"), (5, 33, b"ctc_pruning"), (5, -1, b"ctc_pruning")):
        rc = L.cn_op_ctc_ngram_beam(C.byref(lm.desc(lm.device)), _ptr(logp), _ptr(top), _ptr(ratio), B, Tp, V, W, P, 0.0, 0.5, 0, _ptr(d.hyp),
                                    Tp + 1, _ptr(d.hlen), _ptr(d.sc), _ptr(d.slm), _ptr(d.pb), _ptr(d.pnb), _ptr(d.nb), hip.current_stream())
        assert rc != 0 and msg in L.cn_last_error()
    torch.cuda.synchronize()
    assert (d.hyp.cpu().numpy() == cases.SENT_I).all() and (d.slm.cpu().numpy() == cases.SENT_F).all() and (d.nb.cpu().numpy() == cases.SENT_I).all()
