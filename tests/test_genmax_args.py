"""The descriptor entry of the fused generator tail (cn_op_genmax_desc), the host-only query of the kernel a call takes
(cn_genmax_form) and their argument checks, in both libraries.  No device needed: every call below is refused, or decided, before
anything is sized, packed, uploaded or launched.  The kernels themselves are compared with a float64 model in test_gpu_genmax.py."""
import ctypes as C

import numpy as np
import pytest

import genmax_model as gx
from cassnat_asr_public_amd import abi, hip

K_ = abi.CONSTANTS
FLAVOURS = [None, "f16"]
OWN16 = {None: K_["CN_PRECISION_BF16"], "f16": K_["CN_PRECISION_F16"]}
X3 = K_["CN_PRECISION_BF16X3"]
# a host buffer stands in for every pointer: the calls under test never get as far as following one
_BUF = np.zeros(1 << 12, np.float32)
P = _BUF.ctypes.data
ENTRIES = ("cn_op_genmax_desc", "cn_genmax_desc_size", "cn_genmax_form", "cn_genmax_form_launch", "cn_genmax_pack")


def desc(flavour=None, **kw):
    """An arg-max + maxlp call of the library's own 16-bit operand the entry would accept, with ``kw`` overriding fields."""
    f = dict(precision=OWN16[flavour], reserved=0, h_dev=P, w_host=P, b_host=P, M=10, V=40, arg_dev=P, maxlp_dev=P)
    f.update(kw)
    return hip.CnGenmaxDesc(**f)


def gather(flavour=None, **kw):
    return desc(flavour, **dict(dict(arg_dev=None, maxlp_dev=None, tgt_dev=P, tgt_lp_dev=P, U=5, ld=6), **kw))


def refused(L, d, *words):
    for fn, name in ((lambda p: L.cn_op_genmax_desc(p, None), "cn_op_genmax_desc"), (L.cn_genmax_form, "cn_genmax_form")):
        rc = fn(C.byref(d) if d is not None else None)
        msg = L.cn_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert msg.startswith(name + ": "), msg
        for w in words:
            assert w in msg, (w, msg)


def test_entry_points_are_declared_exported_and_sized_like_the_c_struct():
    assert sorted(abi.GENMAX_FUNCTIONS) == sorted(ENTRIES) and not set(ENTRIES) & set(abi.FUNCTIONS)
    assert {"cn_op_genmax", "cn_op_genmax_gather", "cn_op_genmax_x3"} <= set(hip.declared_symbols())
    for flavour in FLAVOURS:
        L = hip.lib(flavour)
        for name in ENTRIES:
            fn = getattr(L, name)
            assert fn.restype is abi.GENMAX_FUNCTIONS[name][0] and list(fn.argtypes) == abi.GENMAX_FUNCTIONS[name][1], name
        assert L.cn_genmax_desc_size() == C.sizeof(hip.CnGenmaxDesc) == 88
    assert hip.CnGenmaxDesc is abi.GENMAX_STRUCTS["cn_genmax_desc"]
    assert [n for n, _ in hip.CnGenmaxDesc._fields_] == ["precision", "reserved", "h_dev", "w_host", "b_host", "M", "V", "arg_dev", "maxlp_dev",
                                                        "m_dev", "tgt_dev", "U", "ld", "tgt_lp_dev"]
    assert [abi.GENMAX_CONSTANTS["CN_GENMAX_KIND_" + n] for n in ("ARGMAX_LSE", "ARGMAX", "GATHER")] == [0, 1, 2]  # the values of kernels.h


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_what_the_issue_lists(flavour):
    L = hip.lib(flavour)
    d = lambda **kw: desc(flavour, **kw)
    g = lambda **kw: gather(flavour, **kw)
    refused(L, None, "null descriptor")
    refused(L, d(reserved=1), "reserved")
    for name in ("h_dev", "w_host", "b_host"):
        refused(L, d(**{name: None}), "null h_dev, w_host or b_host")
    refused(L, d(M=-1), "M=-1", "negative")
    for V in (0, -1, -127, -128, -1000, -(2 ** 31), 6145, 2 ** 31 - 1):
        refused(L, d(V=V), f"V={V}", "6144")
    for prec in (K_["CN_PRECISION_F32"], K_["CN_PRECISION_FP8"], 7, -1):
        refused(L, d(precision=prec), "precision must be")
    # a precision of the other library (cn_own_precision); the split kernel belongs to the default library alone
    refused(L, d(precision=OWN16["f16" if flavour is None else None]), "libcassnat_hip_f16.so")
    if flavour == "f16":
        refused(L, d(precision=X3), "libcassnat_hip_f16.so")
    refused(L, d(arg_dev=None, maxlp_dev=None), "neither")
    refused(L, g(arg_dev=P), "arg and maxlp must be null")
    refused(L, g(maxlp_dev=P), "arg and maxlp must be null")
    refused(L, g(tgt_lp_dev=None), "needs an output buffer")
    refused(L, g(U=0), "U=0")
    refused(L, g(U=-2, ld=-1), "U=-2")
    refused(L, g(U=5, ld=4), "ld=4")
    refused(L, g(M=11), "M=11")
    refused(L, d(arg_dev=None), "maxlp without arg")
    # and what is not refused: every kind, M == 0 included (nothing to launch, no device touched)
    assert gx.form_parts(L.cn_genmax_form(C.byref(d())))[1:3] == (1, gx.KINDS["lse"])
    assert gx.form_parts(L.cn_genmax_form(C.byref(d(maxlp_dev=None))))[1:3] == (1, gx.KINDS["argmax"])
    assert gx.form_parts(L.cn_genmax_form(C.byref(g())))[1:3] == (1, gx.KINDS["gather"])
    for zero in (d(M=0), g(M=0)):
        assert gx.form_parts(L.cn_genmax_form(C.byref(zero)))[1] == 0
        assert L.cn_op_genmax_desc(C.byref(zero), None) == 0


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_old_entry_points_refuse_with_a_message_and_not_with_an_exception(flavour):
    """cn_op_genmax and cn_op_genmax_gather sized their vectors from genmax_vtw(V) before anything looked at V: integer division
    makes that negative for V <= -128 and the allocation threw through extern "C"; null pointers were followed.  cn_op_genmax_x3
    answered M < 1 with "V too large"."""
    L = hip.lib(flavour)

    def no(rc, who, *words):
        msg = L.cn_last_error().decode()
        assert rc == -1 and msg.startswith(who + ": "), (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    for V in (-1000, 0, 6145):
        no(L.cn_op_genmax(P, P, P, 10, V, P, P, None), "cn_op_genmax", f"V={V}", "6144")
        no(L.cn_op_genmax_gather(P, P, P, 2, 5, V, P, 6, P, None), "cn_op_genmax_gather", f"V={V}", "6144")
    for i in range(3):
        args = [P, P, P]
        args[i] = None
        no(L.cn_op_genmax(*args, 10, 40, P, P, None), "cn_op_genmax", "null h_dev, w_host or b_host")
        no(L.cn_op_genmax_gather(*args, 2, 5, 40, P, 6, P, None), "cn_op_genmax_gather", "null h_dev, w_host or b_host")
    no(L.cn_op_genmax(P, P, P, 10, 40, None, None, None), "cn_op_genmax", "neither")
    no(L.cn_op_genmax(P, P, P, 10, 40, None, P, None), "cn_op_genmax", "maxlp without arg")
    no(L.cn_op_genmax(P, P, P, -3, 40, P, P, None), "cn_op_genmax", "negative")
    no(L.cn_op_genmax_gather(P, P, P, 2, 5, 40, None, 6, P, None), "cn_op_genmax_gather", "neither")
    no(L.cn_op_genmax_gather(P, P, P, 2, 5, 40, P, 6, None, None), "cn_op_genmax_gather", "needs an output buffer")
    no(L.cn_op_genmax_gather(P, P, P, 2, 5, 40, P, 4, P, None), "cn_op_genmax_gather", "ld=4")
    no(L.cn_op_genmax_gather(P, P, P, -1, 5, 40, P, 6, P, None), "cn_op_genmax_gather")
    no(L.cn_op_genmax_gather(P, P, P, 2, 0, 40, P, 6, P, None), "cn_op_genmax_gather")
    no(L.cn_op_genmax_gather(P, P, P, 1 << 20, 1 << 12, 40, P, 1 << 12, P, None), "cn_op_genmax_gather")  # (B x U past int32)
    assert L.cn_op_genmax(P, P, P, 0, 40, P, P, None) == 0 and L.cn_op_genmax_gather(P, P, P, 0, 5, 40, P, 6, P, None) == 0
    x3 = lambda *a: L.cn_op_genmax_x3(*a)
    if flavour == "f16":
        no(x3(P, P, P, 10, 40, P, P, None, 0, 0, None, None), "cn_op_genmax_x3", "libcassnat_hip_f16.so")
        return
    for V in (-1000, 0, 6145):
        no(x3(P, P, P, 10, V, P, P, None, 0, 0, None, None), "cn_op_genmax_x3", f"V={V}", "6144")
    for i in range(3):
        args = [P, P, P]
        args[i] = None
        no(x3(*args, 10, 40, P, P, None, 0, 0, None, None), "cn_op_genmax_x3", "null h_dev, w_host or b_host")
    no(x3(P, P, P, -1, 40, P, P, None, 0, 0, None, None), "cn_op_genmax_x3", "negative")
    no(x3(P, P, P, 10, 40, None, None, None, 0, 0, None, None), "cn_op_genmax_x3", "neither")
    no(x3(P, P, P, 10, 40, None, None, P, 5, 4, P, None), "cn_op_genmax_x3", "ld=4")
    assert x3(P, P, P, 0, 40, P, P, None, 0, 0, None, None) == 0  # (was: "V too large")


# ---- coverage: the instantiations genmax.hip compiles (launch_genmax), as (kernel, 32-row tiles, kind).  The fp16 library compiles
# the same sources and owns CN_PRECISION_F16 alone (cn_own_precision): the 16-bit kernel's six forms are all it can be asked for.
SIX = lambda kernel: {(gx.KERNEL_CODE[kernel], mt, kind) for mt in (1, 2) for kind in gx.KINDS.values()}
INSTANTIATIONS = {None: SIX("16") | SIX("split"), "f16": SIX("16")}


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_launches_reach_every_instantiation_and_each_runs_the_one_it_claims(flavour):
    L = hip.lib(flavour)
    other = hip.lib("f16" if flavour is None else None)
    reached = set()
    lds, grid = C.c_int32(-1), C.c_int32(-1)
    for c, layout, kind, mode in gx.LAUNCHES:
        d = gx.descriptor(c, layout, kind, lambda name: P)
        mine = gx.LAYOUTS[layout][0] == flavour
        own = L if mine else other
        code = own.cn_genmax_form_launch(C.byref(d), C.byref(lds), C.byref(grid))
        assert code == gx.form_code(c["M"], c["V"], layout, kind) == own.cn_genmax_form(C.byref(d)), (gx.launch_id(c, layout, kind, mode), own.cn_last_error())
        kernel, mt, _, vtw = gx.form_parts(code)
        assert lds.value == gx.lds_bytes(gx.LAYOUTS[layout][3], mt, vtw) <= 160 * 1024 and grid.value == -(-c["M"] // (32 * mt))
        # the query is the authority on which library runs a layout: the other one refuses it
        assert (other if mine else L).cn_genmax_form(C.byref(d)) == -1, gx.launch_id(c, layout, kind, mode)
        if mine:
            reached.add(gx.form_parts(code)[:3])
    assert reached == INSTANTIATIONS[flavour], (sorted(INSTANTIATIONS[flavour] - reached), sorted(reached - INSTANTIATIONS[flavour]))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_thresholds_sit_where_the_code_puts_them(flavour):
    L = hip.lib(flavour)
    for kind, d in (("lse", desc), ("argmax", lambda f, **kw: desc(f, maxlp_dev=None, **kw)), ("gather", lambda f, **kw: gather(f, U=1, ld=1, **kw))):
        for M, mt in ((1, 1), (32, 1), (33, 2), (64, 2), (65, 2), (1 << 20, 2)):
            assert gx.form_parts(L.cn_genmax_form(C.byref(d(flavour, M=M)))) == (gx.KERNEL_CODE["16"], mt, gx.KINDS[kind], 2), (kind, M)
        if flavour is None:
            for M, mt in ((1, 1), (33, 1), (8192, 1), (8193, 2), (8225, 2)):
                assert gx.form_parts(L.cn_genmax_form(C.byref(d(flavour, precision=X3, M=M)))) == (gx.KERNEL_CODE["split"], mt, gx.KINDS[kind], 1), (kind, M)
    # tiles per wave: the 16-bit kernel rounds up to even, the split kernel does not; 6144 is the last vocabulary either takes
    for V, v16, v3 in ((1, 2, 1), (128, 2, 1), (129, 2, 1), (256, 2, 1), (257, 4, 2), (384, 4, 2), (1028, 10, 5), (4234, 34, 17), (6144, 48, 24)):
        assert gx.form_parts(L.cn_genmax_form(C.byref(desc(flavour, V=V))))[3] == v16 == gx.vtw_of("16", V)
        if flavour is None:
            assert gx.form_parts(L.cn_genmax_form(C.byref(desc(flavour, precision=X3, V=V))))[3] == v3 == gx.vtw_of("split", V)
