"""The descriptor entry of the row-chain kernel (cn_op_chain_desc) and its argument checks.  No device needed: every call below must
be refused before the weights are packed and anything is launched.  The kernel itself is compared with a float64 model in
test_gpu_chain.py."""
import ctypes as C

import numpy as np
import pytest

from cassnat_asr_public_amd import hip

FLAVOURS = [None, "f16"]
# a host buffer stands in for every pointer: the calls under test never get as far as reading one
_BUF = np.zeros(1 << 16, np.float32)
P = _BUF.ctypes.data
WEIGHTS = dict(wo=P, bo=P, ln1_a=P, ln1_b=P, w1=P, b1=P, w2=P, b2=P, nln_a=P, nln_b=P, wt=P, bt=P)


def desc(**kw):
    """An encoder layer's launch the kernel would accept, with ``kw`` overriding fields."""
    f = dict(x=P, ctx=P, ldctx=256, out=P, ldo=768, M=10, dff=2048, tail_n=768, eps=1e-6, store_x=1, **WEIGHTS)
    f.update(kw)
    return hip.CnChainDesc(**f)


def refused(L, d, *words):
    rc = L.cn_op_chain_desc(C.byref(d) if d is not None else None, None)
    msg = L.cn_last_error().decode()
    assert rc != 0, msg
    assert msg.startswith("cn_op_chain_desc: "), msg
    for w in words:
        assert w in msg, (w, msg)


def test_descriptor_entry_is_declared_exported_and_sized_like_the_c_struct():
    names = hip.declared_symbols()
    for name in ("cn_op_chain_desc", "cn_chain_desc_size", "cn_op_chain", "cn_op_chain_rows"):
        assert name in names
        for flavour in FLAVOURS:
            getattr(hip.lib(flavour), name)
    for flavour in FLAVOURS:
        assert hip.lib(flavour).cn_chain_desc_size() == C.sizeof(hip.CnChainDesc)
    # every field of cn_op_chain_rows, and what it could not reach, in the header's order
    assert [n for n, _ in hip.CnChainDesc._fields_] == [
        "x", "ctx", "ldctx", "ctx_blocked", "wo", "bo", "ln1_a", "ln1_b", "w1", "b1", "w2", "b2", "nln_a", "nln_b", "wt", "bt", "out",
        "ln_out", "ldo", "ld_ln", "M", "dff", "tail_n", "eps", "ln_blocked", "out_blocked", "store_x", "x_in_blocked", "x_out_blocked",
        "swish", "f8", "rows_dev"]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_what_the_issue_lists(flavour):
    L = hip.lib(flavour)
    refused(L, None, "null descriptor")
    refused(L, desc(ctx_blocked=1, ldctx=288), "blocked ctx", "256")
    refused(L, desc(tail_n=0, ldo=256, ln_blocked=1, ln_out=P, ld_ln=288), "blocked LNn(x)", "256")
    refused(L, desc(tail_n=0, ldo=288, ln_blocked=1), "blocked LNn(x)", "256")  # (`out` takes LNn(x): its stride is ldo)
    refused(L, desc(out=None), "a tail needs")
    refused(L, desc(nln_a=None, nln_b=None), "a tail needs")
    refused(L, desc(rows_dev=P, swish=1), "device-side row count", "ReLU")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_bad_geometry_and_missing_weights(flavour):
    L = hip.lib(flavour)
    for dff in (-128, 64, 2048 + 128):
        refused(L, desc(dff=dff), "multiple of 128")
    for tail in (-256, 128, 1536 + 256):
        refused(L, desc(tail_n=tail, ldo=2048), "multiple of 256")
    refused(L, desc(x=None), "null x")
    refused(L, desc(wo=None), "ctx needs wo and bo")
    refused(L, desc(w2=None), "d_ff > 0 needs")
    refused(L, desc(nln_b=None), "nln_a needs nln_b")
    refused(L, desc(wt=None), "a tail needs")
    refused(L, desc(tail_n=0, out=None), "LNn(x) needs out or ln_out")
    refused(L, desc(tail_n=0, nln_a=None, nln_b=None, ln_out=P, ld_ln=256), "ln_out needs")
    refused(L, desc(f8=1, dff=128), "e4m3", "d_ff % 256")
    refused(L, desc(f8=1, swish=1), "e4m3", "ReLU")
    # rows the vector loads and stores can address: 256 / tail_n columns at the least, 16-byte (LNn(x): 8-byte) aligned
    refused(L, desc(ldctx=128), "ldctx >= 256")
    refused(L, desc(ldctx=260), "ldctx >= 256")
    refused(L, desc(ldo=512), "ldo >= tail_n")
    refused(L, desc(ldo=772), "16-byte")
    refused(L, desc(out_blocked=1, ldo=768 + 16), "ldo % 32")
    refused(L, desc(tail_n=0, ldo=128), "ld >= 256")
    refused(L, desc(ln_out=P, ld_ln=258), "8-byte")
    refused(L, desc(M=-1), "M < 0")
