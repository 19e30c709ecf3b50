"""The split-bf16 engine's own two kernels against the float64 model of x3_model.py, one launch per case: the d_model-deep
projection (csrc/proj_x3.hip) through cn_op_proj_x3_desc - A on the device, every stride the case's - and the fused feed-forward
sublayer with its row-chain forms (csrc/fused_x3.hip) through cn_op_ffn_x3_act and cn_op_x3_chain, in the library that owns the
split precision.  The cases are x3_model.CASES (the case id names the call site or the edge); test_x3_model.py shows on the CPU
what the checks catch, test_x3_args.py that the case list reaches all 4 + 9 instantiations.

Per launch (x3_model.check_launch): the guards (inputs, sentinels and NaN rows bit for bit as before, xn_out finite where it is
written and untouched where it is not), |out - fp64| <= bound on every live element, rms(out - fp64) within RATIO of the
emulation's.  Before the launch the form queries must name the instantiation the case is written for.

Run with -s to see the worst ratios per form (the tables of docs/KERNEL_NOTES.md) and every case's rms error."""
import ctypes as C

import pytest
import torch

import x3_model as xm
from attention_model import LAYOUTS
from cassnat_asr_public_amd import abi, hip

pytestmark = pytest.mark.gpu

WORST = {}
ACT = {False: abi.CONSTANTS["CN_ACT_RELU"], True: abi.CONSTANTS["CN_ACT_SWISH"]}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |out - fp64| / bound and rms(out - fp64) / yardstick per form and output:")
    for (form, name), (b, r) in sorted(WORST.items()):
        print(f"  {form:22s} {name:4s} {b:.3f}  {r:.3f}")
    for fam in sorted(xm.RATIO):
        rs = [r for f, r in FAMILY if f == fam]
        if rs:
            print(f"  {fam}: worst rms ratio {max(rs):.4f} (allowed {xm.RATIO[fam]})")
    xm._MODEL.clear()


FAMILY = []


def library():
    flavour, _, operand = LAYOUTS[xm.LAYOUT]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    return L


def launch(c, host):
    """One call on device copies of the case's host buffers; returns them afterwards (host)."""
    L = library()
    host_side = ("wo", "w1", "w2", "wt") if c["kind"] == "ffn" else ("wt", "bt")
    dev = {k: v.cuda() for k, v in host.items() if k not in host_side}
    hp = lambda k: C.c_void_p(host[k].data_ptr())
    p = lambda k: C.c_void_p(dev[k].data_ptr())
    at = lambda k: C.c_void_p(dev[k].data_ptr() + xm.GR * dev[k].shape[1] * dev[k].element_size())  # behind the guard rows
    if c["kind"] == "proj":
        mt, ch = C.c_int32(), C.c_int32()
        assert L.cn_proj_x3_form(c["M"], c["N"], int(c["split"]), C.byref(mt), C.byref(ch)) == 0
        assert xm.form_name(c, mt.value) == xm.form_name(c)
        resid = None if not c["resid"] else at("C" if c["resid"] == "alias" else "resid")
        d = hip.CnProjX3Desc(a_dev=at("A"), w_host=hp("wt"), bias_host=hp("bt"), c_dev=at("C"), resid_dev=resid, lda=c["lda"], ldc=c["ldc"],
                             ldr=c["ldr"] if c["resid"] else 0, M=c["M"], N=c["N"], split_out=int(c["split"]), resid_scale=c["rs"],
                             reserved=0)
        hip.check(L.cn_op_proj_x3_desc(C.byref(d), hip.current_stream()), "cn_op_proj_x3_desc", L)
    else:
        f = C.c_int32()
        assert L.cn_ffn_x3_form(int(c["ctx"]), c["tail"], int(c["mix"]), ACT[c["swish"]], C.byref(f)) == 0 and f.value == xm.form_bits(c)
        nxt = c["has_next"]
        if not c["ctx"] and not c["tail"]:
            rc = L.cn_op_ffn_x3_act(at("x"), p("a1"), p("b1n"), hp("w1"), p("b1"), hp("w2"), p("b2"), p("na") if nxt else None,
                                    p("nb") if nxt else None, at("xn"), c["M"], c["dff"], 1e-6, int(c["mix"]), ACT[c["swish"]],
                                    hip.current_stream())
            hip.check(rc, "cn_op_ffn_x3_act", L)
        else:
            rc = L.cn_op_x3_chain(at("x"), at("ctx") if c["ctx"] else None, hp("wo"), p("bo"), p("a1"), p("b1n"), hp("w1"), p("b1"),
                                  hp("w2"), p("b2"), p("na") if nxt else None, p("nb") if nxt else None, at("xn"),
                                  hp("wt") if c["tail"] else None, p("bt"), at("tail") if c["tail"] else None, c["tail"], c["M"], c["dff"],
                                  1e-6, int(c["mix"]), hip.current_stream())
            hip.check(rc, "cn_op_x3_chain", L)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in dev.items()}
    out.update({k: host[k] for k in host_side if k in host})
    return out


@pytest.mark.parametrize("c", xm.CASES, ids=[xm.case_id(c) for c in xm.CASES])
def test_launch_against_float64(c):
    before = xm.buffers(c)
    pristine = {k: v.clone() for k, v in before.items()}
    after = launch(c, before)
    seen = {}
    try:
        xm.check_launch(c, pristine, after, seen)
    finally:
        form = xm.form_name(c)
        for name, (b, r, dev) in seen.items():
            print(f"{c['name']} {name}: |err| / bound {b:.3f}, rms / yardstick {r:.4f}, rms error {dev:.3e}")
            old = WORST.get((form, name), (0.0, 0.0))
            WORST[(form, name)] = (max(old[0], b), max(old[1], r))
            FAMILY.append((xm.family(c), r))
