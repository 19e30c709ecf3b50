"""The bias search kernel alone (csrc/ctc_beam.hip, through cn_op_ctc_bias_beam) against cn_ctc_bias_beam_host, the serial host loop
over the same step functions (itself compared with the float64 model in tests/test_ctc_bias_host.py), on that file's shapes and phrase
sets, in both libraries: hypotheses and order exact, score_lm bit for bit (dyadic scores), score_ctc / p_blk / p_nblk to 1e-8 (libm's
and the device's log1p / exp may differ in the last bits); 8 elements behind every output stay untouched.  With the empty list the
kernel is cn_op_ctc_prefix_beam's, another instantiation of the same body: equal bits."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_bias_cases as cases
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import _ptr

pytestmark = pytest.mark.gpu


def run_device(case, flavour=None, bias=None):
    bias = (bias or cases.bias_of(case.name)).cuda()
    B, Tp, V = case.logp.shape
    cap = Tp + 1
    o = cases.outputs(B, case.W, cap)
    d = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(o).items()})
    d.logp, d.ratio = torch.from_numpy(case.logp).cuda(), torch.from_numpy(case.ratio).cuda()
    d.top = torch.from_numpy(np.ascontiguousarray(case.top)).cuda() if case.P else None
    L = hip.lib(flavour)
    rc = L.cn_op_ctc_bias_beam(*cases.call_args(case, bias.desc(bias.device), None, cap, dev=d), hip.current_stream())
    assert rc == 0, L.cn_last_error()
    torch.cuda.synchronize()
    o = SimpleNamespace(**{k: getattr(d, k).cpu().numpy() for k in vars(o)})
    assert cases.untouched(o, B, case.W, cap)
    return cases.beams_of(o, B, case.W, cap)


@functools.lru_cache(maxsize=None)
def host_of(*a):
    """The host entry's beams of make_case(*a), computed once for both libraries."""
    return cases.run_host(cases.make_case(*a))


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("name", list(cases.SETS))
@pytest.mark.parametrize("beam,pruning", cases.BEAMS)
@pytest.mark.parametrize("Tp", cases.SHAPES)
def test_kernel_is_the_host_search(Tp, beam, pruning, name, flavour):
    case = cases.make_case(Tp, beam, pruning, name)
    got = run_device(case, flavour)
    cases.same_beams(got, host_of(Tp, beam, pruning, name))
    assert [e["hyp"] for e in got[2]] == [[]] and got[2][0]["score_lm"] == 0.0  # every frame blank: the empty hypothesis, nothing banked
    if name != "none" and Tp == 40 and beam >= 5:
        assert any(e["score_lm"] != 0.0 for seqs in got for e in seqs)


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("name", ["long", "repeat", "ties_shared_prefix", "ties_negative", "ties_probe_wrap", "pruning0", "foreign"])
def test_kernel_on_the_crafted_cases(name, flavour):
    if name == "long":
        case = cases.long_case()
    elif name == "repeat":
        case = cases.repeat_case()
    elif name.startswith("ties_"):
        case = cases.ties_case(name[5:])
    elif name == "pruning0":
        case = cases.make_case(12, 2, 0, "one_piece")
    else:  # labels outside [0, V) in the pruned lists make no candidate
        case = SimpleNamespace(**vars(cases.make_case(12, 5, 3, "interior")))
        case.P = 5
        case.top = np.concatenate([np.full(case.top.shape[:2] + (1,), cases.V, np.int32), case.top,
                                   np.full(case.top.shape[:2] + (1,), -3, np.int32)], axis=2)
    got = run_device(case, flavour)
    cases.same_beams(got, cases.run_host(case))
    if name == "long":
        assert got[0][0]["hyp"] == case.path and got[0][0]["score_lm"] == 16.0
    if name == "repeat":
        assert got[0][0]["hyp"] == case.labels and got[0][0]["score_lm"] == 17.0


@pytest.mark.parametrize("nodes", [None, 0, 1])
@pytest.mark.parametrize("Tp,W,P,lp", [(1, 1, 1, 0.0), (12, 5, 3, 0.25), (40, 32, 8, 0.1), (40, 32, 27, 0.0), (12, 2, 0, 0.3)])
def test_with_the_empty_list_it_is_the_prefix_beam_kernel(Tp, W, P, lp, nodes):
    """Random log-posteriors (no two equal in a row, so the device's top-k and the list given here are the same).  ``nodes`` None: the
    tables of an empty list; 0 / 1: a descriptor without tables."""
    case = SimpleNamespace(**vars(cases.make_case(Tp, W, P, "none", lp=lp)))
    case.logp = case.logp.copy()
    assert all(len(set(row.tolist())) == cases.V for row in case.logp[:2].reshape(-1, cases.V))
    case.logp[2] = case.logp[0][::-1]  # (the prefix beam kernel's top-k has no rule for the all-blank utterance's equal values)
    case.top = cases.topk_lists(case.logp, case.P)
    if nodes is None:
        got = run_device(case)
    else:
        bias = SimpleNamespace(device="cuda", cuda=lambda: bias)
        d = hip.CnBiasDesc()
        d.slots, d.nodes, d.hash_bits = 1, nodes, 32
        bias.desc = lambda dev: d
        got = run_device(case, bias=bias)
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
            # (one kernel body, one instantiation per fusion policy: the same bits)
            assert e["score_ctc"] == sc[b, j] and e["p_blk"] == pb[b, j] and e["p_nblk"] == pnb[b, j]


def test_refusals_leave_the_outputs_alone():
    bias = cases.bias_of("interior").cuda()
    case = cases.make_case(12, 5, 3, "interior")
    B, Tp, V = case.logp.shape
    o = cases.outputs(B, 5, Tp + 1, pad=0)
    d = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in vars(o).items()})
    logp, ratio, top = (torch.from_numpy(a).cuda() for a in (case.logp, case.ratio, case.top))
    L = hip.lib()
    good = bias.desc(bias.device)
    odd = hip.CnBiasDesc()
    C.memmove(C.byref(odd), C.byref(good), C.sizeof(odd))
    odd.slots = good.slots - 1
    for desc, W, P, msg in ((good, 0, 3, b"ctc_beam"), (good, 33, 3, b"ctc_beam"), (good, 5, 33, b"ctc_pruning"), (good, 5, -1, b"ctc_pruning"),
                            (odd, 5, 3, b"power of two")):
        rc = L.cn_op_ctc_bias_beam(C.byref(desc), _ptr(logp), _ptr(top), _ptr(ratio), B, Tp, V, W, P, 0.0, 0, _ptr(d.hyp), Tp + 1, _ptr(d.hlen),
                                   _ptr(d.sc), _ptr(d.slm), _ptr(d.pb), _ptr(d.pnb), _ptr(d.nb), hip.current_stream())
        assert rc != 0 and msg in L.cn_last_error()
    torch.cuda.synchronize()
    assert (d.hyp.cpu().numpy() == cases.SENT_I).all() and (d.slm.cpu().numpy() == cases.SENT_F).all() and (d.nb.cpu().numpy() == cases.SENT_I).all()
