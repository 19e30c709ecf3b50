"""The edit-alignment kernel (cn_op_edit_align) against the host entry and the model (tests/edit_model.py): cost, counts, path length and
every byte of the paths over the whole case list, with the back-pointers in LDS and in device scratch, in both libraries; sentinels
behind every path, every ops span and row N survive; the threshold between the two forms; the Python entry on torch tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import edit_cases
from cassnat_asr_public_amd import hip
from test_edit_host import host_call

pytestmark = pytest.mark.gpu

KEYS = ("ref", "ref_begin", "ref_len", "hyp", "hyp_begin", "hyp_len", "ops_begin", "cost", "counts", "path_len", "ops")


def p(t):
    return C.c_void_p(t.data_ptr())


def device_call(L, limit):
    def call(a):
        d = {k: torch.from_numpy(a[k]).cuda() for k in KEYS}
        rc = L.cn_op_edit_align(p(d["ref"]), a["ref_total"], p(d["ref_begin"]), p(d["ref_len"]), p(d["hyp"]), a["hyp_total"], p(d["hyp_begin"]),
                                p(d["hyp_len"]), a["N"], a["max_ref"], a["max_hyp"], *a["costs"], int(limit), p(d["cost"]), p(d["counts"]),
                                p(d["path_len"]), p(d["ops"]), a["ops_total"], p(d["ops_begin"]), hip.current_stream())
        torch.cuda.synchronize()
        for k in ("cost", "counts", "path_len", "ops"):
            a[k][...] = d[k].cpu().numpy()
        return rc
    return call


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("limit", [-1, 0], ids=["lds", "scratch"])
@pytest.mark.parametrize("name", [c["name"] for c in edit_cases.cases()])
def test_kernel_equals_the_host_entry_and_the_model(name, limit, flavour):
    case, L = edit_cases.by_name(name), hip.lib(flavour)
    assert edit_cases.run_entry(case, host_call(L)) == []
    assert edit_cases.run_entry(case, device_call(L, limit)) == []


@pytest.mark.parametrize("name", ["n3-433", "widths-111", "n70-shared-123"])
def test_threshold_between_the_two_forms(name):
    """At (max_ref + 1) * (max_hyp + 1) the back-pointers are still in LDS, one below they go to scratch: the same bytes on either side."""
    case = edit_cases.by_name(name)
    at = (case["max_ref"] + 1) * (case["max_hyp"] + 1)
    for limit in (at, at - 1, 1 << 40):
        assert edit_cases.run_entry(case, device_call(hip.lib(), limit)) == [], limit


def test_python_entry_on_torch_tensors():
    case = edit_cases.by_name("n70-shared-433")
    t = lambda k, dt: torch.tensor(case[k], dtype=dt).cuda()
    got = hip.edit_align(t("ref", torch.int32), t("ref_begin", torch.int64), t("ref_len", torch.int32), t("hyp", torch.int32), t("hyp_begin", torch.int64),
                         t("hyp_len", torch.int32), case["costs"])
    cost, counts, plen, ops, ob = (x.cpu().numpy() for x in got)
    w_cost, w_counts, w_plen, w_paths = edit_cases._expected(case["name"])
    assert cost.tolist() == w_cost and counts.tolist() == w_counts and plen.tolist() == w_plen
    assert [ops[b:b + n].tolist() for b, n in zip(ob, plen)] == w_paths
    with pytest.raises(hip.HipError, match="costs must"):
        hip.edit_align(t("ref", torch.int32), t("ref_begin", torch.int64), t("ref_len", torch.int32), t("hyp", torch.int32), t("hyp_begin", torch.int64),
                       t("hyp_len", torch.int32), (1, 0, 1))
