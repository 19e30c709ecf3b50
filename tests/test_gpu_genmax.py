"""The fused generator tail (csrc/genmax.hip: genmax_kernel and genmax_x3_kernel) in every instantiation and launch form, in both
libraries, against the float64 model of genmax_model.py.  Every launch goes through cn_op_genmax_desc, which reaches all of
GenmaxArgs (the device-side row count m_dev included); the launches are genmax_model.LAUNCHES, and test_genmax_model.py shows on the
CPU what the checks catch.  cn_genmax_form must name the instantiation each launch is written for before it runs
(test_genmax_args.py shows that the launches reach every one).

Per launch (genmax_model.check_launch): the arg-max exact on every decided row, a candidate on the others and the lowest of planted
bit-identical entries; |maxlp - fp64| and |tgt_lp - fp64| within the derived bound (never above the older tests' allowance); -inf
exactly for a target outside the vocabulary; and everything the launch does not own bit for bit as before - rows at or past the
count, columns U .. ld, the guards around every buffer (NaN or a sentinel), every input.

Run with -s to see the worst ratios per library, kernel, rows per workgroup and output kind (the table of docs/KERNEL_NOTES.md) and
the measure FAST is set from."""
import ctypes as C

import numpy as np
import pytest
import torch

import genmax_model as gx
from cassnat_asr_public_amd import hip

pytestmark = pytest.mark.gpu

WORST = {}
PAIRS = [(c, layout) for c in gx.CASES for layout in c["layouts"]]


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |maxlp - fp64| / bound, |tgt_lp - fp64| / bound, (|err| - derived) / unit and undecided rows per library, kernel, "
          "32-row tiles per workgroup and output kind:")
    for key, w in sorted(WORST.items()):
        print("  %-5s %-6s mt %d %-7s" % key + "  maxlp %.4f  tgt %.4f  fast %+.3f  undecided %.4f" % (w["maxlp"], w["tgt"], w["fast"], w["undecided"]))
    if WORST:
        print(f"  worst (|err| - derived) / unit over all launches: {max(w['fast'] for w in WORST.values()):+.4f}  (FAST_MEASURED "
              f"{gx.FAST_MEASURED}, asserted FAST {gx.FAST})")
    gx._MODEL.clear()
    gx._RAW.clear()


def lib_of(layout):
    flavour, _, operand, _ = gx.LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    return L


def launch(c, layout, kind, host):
    """One cn_op_genmax_desc call on device copies of the launch's buffers (W and b stay on the host); returns them afterwards."""
    L = lib_of(layout)
    dev = {k: (torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() if v is not None and k not in ("W", "b") else v)
           for k, v in host.items()}

    def address(name):
        if name in ("W", "b"):
            return dev[name].ctypes.data
        return dev[name].data_ptr() + gx.GUARD * dev[name].element_size()

    d = gx.descriptor(c, layout, kind, address)
    assert L.cn_genmax_form(C.byref(d)) == gx.form_code(c["M"], c["V"], layout, kind), (L.cn_genmax_form(C.byref(d)), L.cn_last_error())
    hip.check(L.cn_op_genmax_desc(C.byref(d), hip.current_stream()), "cn_op_genmax_desc", L)
    torch.cuda.synchronize()
    back = lambda k, v: v if v is None or k in ("W", "b") else (v.cpu().numpy().view(np.uint16) if host[k].dtype == np.uint16 else v.cpu().numpy())
    return {k: back(k, v) for k, v in dev.items()}


@pytest.mark.parametrize("c, layout", PAIRS, ids=[f"{c['name']}@{layout}" for c, layout in PAIRS])
def test_launches_against_float64(c, layout):
    kernel = gx.LAYOUTS[layout][3]
    for cc, ll, kind, mode in gx.LAUNCHES:
        if cc is not c or ll != layout:
            continue
        before = gx.buffers(c, layout, kind, mode)
        after = launch(c, layout, kind, gx.copy_of(before))
        seen = {}
        try:
            gx.check_launch(c, layout, kind, before, after, seen)
        finally:
            if seen:
                print(f"{gx.launch_id(c, layout, kind, mode)}: maxlp {seen['maxlp']:.4f}  tgt {seen['tgt']:.4f} of the bound, "
                      f"(|err| - derived) / unit {seen['fast']:+.3f}, undecided rows {seen['undecided']:.4f}")
                key = (gx.LAYOUTS[layout][2], kernel, gx.mt_of(kernel, c["M"]), kind)
                old = WORST.setdefault(key, dict(maxlp=0.0, tgt=0.0, fast=-np.inf, undecided=0.0))
                for k in old:
                    old[k] = max(old[k], seen[k])
        assert seen["undecided"] <= (0.0 if c["data"] in gx.PLANTED else gx.UNDECIDED_CAP)


@pytest.mark.parametrize("layout", list(gx.LAYOUTS))
def test_nothing_to_launch_leaves_every_sentinel(layout):
    """M = 0: rc 0 and every buffer untouched, in each output kind."""
    c = gx.BY_NAME[("shape-M33-V1028", layout)]
    L = lib_of(layout)
    for kind in ("lse", "argmax", "gather"):
        host = gx.buffers(c, layout, kind, "mixed" if kind == "gather" else None)
        dev = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for k, v in host.items() if v is not None and k not in ("W", "b")}
        address = lambda name: host[name].ctypes.data if name in ("W", "b") else dev[name].data_ptr() + gx.GUARD * dev[name].element_size()
        d = gx.descriptor(c, layout, kind, address)
        d.M = 0
        assert gx.form_parts(L.cn_genmax_form(C.byref(d)))[1] == 0
        assert L.cn_op_genmax_desc(C.byref(d), hip.current_stream()) == 0
        torch.cuda.synchronize()
        for name, t in dev.items():
            assert np.array_equal(t.cpu().numpy().view(np.uint8), host[name].view(np.uint8)), (kind, name)
