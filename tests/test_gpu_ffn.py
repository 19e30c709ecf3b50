"""The fused feed-forward sublayer (csrc/fused.hip) as cn_op_ffn_fused_act launches it - the whole sublayer in one launch (MT = 1
up to 32 rows, MT = 2 above) and the d_ff split with its reduce kernel that decode_ar.hip's run_ffn_step uses - in both libraries
(bf16 and fp16 operands), ReLU and Swish, with and without the next LayerNorm, against chain_model.py's float64 model.  The cases
are ffn_model.CASES (the case id names the call site); test_ffn_model.py shows on the CPU what the checks catch.

Per launch (ffn_model.check_launch): |out - fp64| <= bound on every live element of x and xn_out, the RMS of (out - fp64) within
RATIO of the emulation's, the sentinel rows around x and xn_out bit for bit as before, xn_out (NaN before the launch) finite in
every live element - or untouched where there is no next LayerNorm.

Run with -s to see the worst ratios per library and form (the table of docs/KERNEL_NOTES.md)."""
import ctypes as C

import pytest
import torch

import chain_model as cm
import ffn_model as fm
from attention_model import LAYOUTS
from cassnat_asr_public_amd import abi, hip

pytestmark = pytest.mark.gpu

WORST = {}
ACT = {False: abi.CONSTANTS["CN_ACT_RELU"], True: abi.CONSTANTS["CN_ACT_SWISH"]}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |out - fp64| / bound and rms(out - fp64) / yardstick per library, form and output:")
    for (layout, form, name), (b, r) in sorted(WORST.items()):
        print(f"  {layout:5s} {form:28s} {name:3s} {b:.3f}  {r:.3f}")
    for layout in fm.LIBS:
        rs = [v for k, v in WORST.items() if k[0] == layout]
        if rs:
            print(f"  {layout}: worst bound ratio {max(b for b, _ in rs):.3f}, worst rms ratio {max(r for _, r in rs):.3f}")
    fm._MODEL.clear()


def launch(c, layout, host):
    flavour, _, operand = LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    w = fm.weights_of(c)
    dev = {k: v.cuda() for k, v in host.items()}
    wd = {k: w[k].cuda() for k in ("a1", "b1n", "b1", "b2", "na", "nb")}
    p = lambda t: C.c_void_p(t.data_ptr())
    at = lambda t: C.c_void_p(t.data_ptr() + fm.GUARD_ROWS * fm.D * t.element_size())
    nxt = c["has_next"]
    rc = L.cn_op_ffn_fused_act(at(dev["x"]), p(wd["a1"]), p(wd["b1n"]), p(w["w1"]), p(wd["b1"]), p(w["w2"]), p(wd["b2"]),
                               p(wd["na"]) if nxt else None, p(wd["nb"]) if nxt else None, at(dev["xn"]), c["M"], c["dff"], 1e-6,
                               c["nslice"], ACT[c["swish"]], hip.current_stream())
    hip.check(rc, "cn_op_ffn_fused_act", L)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev.items()}


@pytest.mark.parametrize("layout", fm.LIBS)
@pytest.mark.parametrize("c", fm.CASES, ids=[fm.case_id(c) for c in fm.CASES])
def test_launch_against_float64(c, layout):
    before = fm.buffers(c, layout)
    after = launch(c, layout, before)
    seen = {}
    try:
        fm.check_launch(c, layout, before, after, seen)
    finally:
        form = f"{'swish' if c['swish'] else 'relu'}-MT{1 if c['M'] <= 32 else 2}-s{c['nslice']}-{'next' if c['has_next'] else 'last'}"
        for name, (b, r) in seen.items():
            print(f"{layout} {c['name']} {name}: |err| / bound {b:.3f}, rms / yardstick {r:.3f}")
            old = WORST.get((layout, form, name), (0.0, 0.0))
            WORST[(layout, form, name)] = (max(old[0], b), max(old[1], r))
