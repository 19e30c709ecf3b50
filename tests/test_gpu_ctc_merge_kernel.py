"""The merging search kernel alone (csrc/ctc_beam.hip, MERGE instantiations, through cn_op_ctc_merged_beam) against
cn_ctc_merged_beam_host - the serial host loop that orders with std::stable_sort and decides identity by comparing label vectors
(itself compared with the float64 model in tests/test_ctc_merge_host.py) - on that file's shapes and cases, in both libraries and for
the three fusion policies: hypotheses and order exact, score_lm bit for bit (dyadic model and scores), score_ctc / p_blk / p_nblk to
1e-8 (libm's and the device's log1p / exp may differ in the last bits); 8 elements behind every output stay untouched.  Where nothing
can fold the kernel is cn_op_ctc_prefix_beam's, and with the empty list the LM-free merged one: equal bits."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_bias_cases
import ctc_merge_cases as cases
import ctc_ngram_cases
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import _ptr

pytestmark = pytest.mark.gpu


def run_device(case, policy, flavour=None, swap=None):
    """``swap`` (ngram desc or None, lm_scale, bias desc or None): other descriptors than the policy's."""
    B, Tp, V = case.logp.shape
    cap = Tp + 1
    o = cases.outputs(B, case.W, cap)
    d = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(o).items()})
    d.logp, d.ratio = torch.from_numpy(case.logp).cuda(), torch.from_numpy(case.ratio).cuda()
    d.top = torch.from_numpy(np.ascontiguousarray(case.top)).cuda() if case.P else None
    L = hip.lib(flavour)
    args, keep = cases.call_args(case, policy, None, cap, dev=d, tables=True)
    if swap is not None:
        ng, scale, bias = swap
        args = (C.byref(ng) if ng is not None else None, scale, C.byref(bias) if bias is not None else None) + args[3:]
    rc = L.cn_op_ctc_merged_beam(*args, hip.current_stream())
    assert rc == 0, L.cn_last_error()
    torch.cuda.synchronize()
    o = SimpleNamespace(**{k: getattr(d, k).cpu().numpy() for k in vars(o)})
    assert cases.untouched(o, B, case.W, cap)
    return cases.beams_of(o, B, case.W, cap)


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("beam,pruning", cases.BEAMS)
@pytest.mark.parametrize("Tp", cases.SHAPES)
def test_kernel_is_the_host_search(Tp, beam, pruning, policy, flavour):
    """Planted paths: one utterance searched over all its frames, one cut short by its size ratio, one whose every frame is skipped."""
    case = cases.make_case(Tp, beam, pruning)
    got = run_device(case, policy, flavour)
    cases.same_beams(got, cases.run_host(case, policy))
    assert [e["hyp"] for e in got[2]] == [[]] and got[2][0]["score_ctc"] == 0.0
    assert policy == "ngram" or got[2][0]["score_lm"] == 0.0  # (the n-gram policy scores </s> behind the empty hypothesis)


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("name", cases.CRAFTED)
def test_kernel_on_the_crafted_cases(name, policy, flavour):
    """Three labels over 40 frames (nearly every frame folds; 5 / 8 and 32 / 32, the latter with more than 256 candidates and with
    folds that no slot link joins), runs of one label, the dropped-and-re-created prefix, duplicate labels in the pruned rows."""
    case = cases.crafted(name)
    got = run_device(case, policy, flavour)
    cases.same_beams(got, cases.run_host(case, policy))
    for seqs in got:
        assert len({tuple(e["hyp"]) for e in seqs}) == len(seqs)


@pytest.mark.parametrize("beam,pruning", [(20, 30), (32, 32)])
def test_many_candidates_of_few_labels(beam, pruning):
    case = cases.alphabet_case(40, beam, pruning, seed=7)
    for policy in cases.POLICIES:
        cases.same_beams(run_device(case, policy), cases.run_host(case, policy))


@pytest.mark.parametrize("Tp,W,P,lp", [(1, 1, 0, 0.0), (12, 1, 0, 0.25), (40, 1, 0, 0.1), (12, 1, 3, 0.0), (40, 3, 0, 0.3)])
def test_with_nothing_to_fold_it_is_the_prefix_beam_kernel(Tp, W, P, lp):
    """Random log-posteriors (no two equal in a row, so the device's top-k and the list given here are the same)."""
    case = SimpleNamespace(**vars(cases.make_case(Tp, W, P, lp=lp)))
    case.logp = case.logp.copy()
    assert all(len(set(row.tolist())) == cases.V for row in case.logp[:2].reshape(-1, cases.V))
    case.logp[2] = case.logp[0][::-1]  # (the prefix beam kernel's top-k has no rule for the all-blank utterance's equal values)
    case.top = cases.topk_lists(case.logp, case.P)
    got = run_device(case, "none")
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
            # (one kernel body: the same bits)
            assert e["score_ctc"] == sc[b, j] and e["p_blk"] == pb[b, j] and e["p_nblk"] == pnb[b, j]


@pytest.mark.parametrize("name", ["abc40", "abc40_wide", "relink", "duplicate"])
def test_with_the_empty_list_it_is_the_lm_free_merged_kernel(name):
    case = cases.crafted(name)
    want = run_device(case, "none")
    empty = ctc_bias_cases.bias_of("none").cuda()
    root = hip.CnBiasDesc()
    root.slots, root.nodes, root.hash_bits = 1, 1, 32
    for bias in (empty.desc(empty.device), root):
        cases.same_beams(run_device(case, "none", swap=(None, 0.0, bias)), want, tol=0.0)


def test_refusals_leave_the_outputs_alone():
    bias = ctc_bias_cases.bias_of(cases.PHRASES).cuda()
    lm = ctc_ngram_cases.lm_of(cases.ORDER)[0].cuda()
    case = cases.make_case(12, 5, 8)
    B, Tp, V = case.logp.shape
    o = cases.outputs(B, 5, Tp + 1, pad=0)
    d = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(o).items()})
    logp, ratio, top = (torch.from_numpy(a).cuda() for a in (case.logp, case.ratio, case.top))
    L = hip.lib()
    good, ng = bias.desc(bias.device), lm.desc(lm.device)
    odd = hip.CnBiasDesc()
    C.memmove(C.byref(odd), C.byref(good), C.sizeof(odd))
    odd.slots = good.slots - 1
    for n, b, W, P, msg in ((None, good, 0, 3, b"ctc_beam"), (None, None, 33, 3, b"ctc_beam"), (ng, None, 5, 33, b"ctc_pruning"),
                            (None, good, 5, -1, b"ctc_pruning"), (None, odd, 5, 3, b"power of two"), (ng, good, 5, 3, b"at most one")):
        rc = L.cn_op_ctc_merged_beam(C.byref(n) if n is not None else None, 0.5, C.byref(b) if b is not None else None, _ptr(logp), _ptr(top),
                                     _ptr(ratio), B, Tp, V, W, P, 0.0, 0, _ptr(d.hyp), Tp + 1, _ptr(d.hlen), _ptr(d.sc), _ptr(d.slm), _ptr(d.pb),
                                     _ptr(d.pnb), _ptr(d.nb), hip.current_stream())
        assert rc != 0 and msg in L.cn_last_error()
    torch.cuda.synchronize()
    assert (d.hyp.cpu().numpy() == cases.SENT_I).all() and (d.slm.cpu().numpy() == cases.SENT_F).all() and (d.nb.cpu().numpy() == cases.SENT_I).all()
