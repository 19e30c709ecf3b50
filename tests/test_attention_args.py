"""The descriptor entry of the fused attention kernel (cn_op_attention_desc) and its argument checks.  No device needed: every call
below must be refused before anything is launched.  The kernel itself is compared with a float64 model in test_gpu_attention.py."""
import ctypes as C

import numpy as np
import pytest

from cassnat_asr_public_amd import hip

FLAVOURS = [None, "f16"]
# a host buffer stands in for every device pointer: the calls under test never get as far as reading one
_BUF = np.zeros(1 << 16, np.float32)
P = _BUF.ctypes.data


def own16(flavour):
    return hip.PRECISION["fp16" if flavour == "f16" else "bf16"]


def desc(**kw):
    """A geometry the kernel would accept (H = 2: rows of 128 elements), with ``kw`` overriding fields."""
    f = dict(Q=P, K=P, V=P, O=P, ldq=128, ldk=128, ldv=128, ldo=128, B=2, H=2, Lq=10, Lk=10, kcap_stride=1, scale=0.125)
    f.update(kw)
    return hip.CnAttnDesc(**f)


def refused(L, prec, d, *words):
    rc = L.cn_op_attention_desc(prec, C.byref(d) if d is not None else None, None)
    msg = L.cn_last_error().decode()
    assert rc != 0, msg
    for w in words:
        assert w in msg, (w, msg)


def test_descriptor_entry_is_declared_exported_and_sized_like_the_c_struct():
    names = hip.declared_symbols()
    for name in ("cn_op_attention_desc", "cn_attn_desc_size"):
        assert name in names
        for flavour in FLAVOURS:
            getattr(hip.lib(flavour), name)
    for flavour in FLAVOURS:
        assert hip.lib(flavour).cn_attn_desc_size() == C.sizeof(hip.CnAttnDesc)
    # every AttnArgs field, in the header's order
    assert [n for n, _ in hip.CnAttnDesc._fields_] == [
        "Q", "K", "V", "O", "ldq", "ldk", "ldv", "ldo", "B", "H", "Lq", "Lk", "keymask", "kv_mod", "kv_index", "klen", "kcap",
        "kcap_stride", "q_blocked", "kv_blocked", "q_col", "k_col", "v_col", "q_n", "kv_n", "o_blocked", "intervals", "iv_stride",
        "causal", "scale", "rel_pos", "rel_u", "rel_v", "rel_R", "ld_pos"]


def layouts(flavour):
    """(precision, split-bf16?) of every layout the library holds."""
    if flavour == "f16":
        return [(own16(flavour), False)]
    return [(hip.PRECISION["fp32"], False), (own16(flavour), False), (hip.PRECISION["bf16x3"], True)]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_rows_narrower_than_the_heads(flavour):
    """ld < 64 H on a row-major operand: head h + 1 of a row would be head h's tail of the next row."""
    L = hip.lib(flavour)
    for prec, _ in layouts(flavour):
        for field in ("ldq", "ldk", "ldv", "ldo"):
            refused(L, prec, desc(**{field: 96}), "64 * H")
        refused(L, prec, desc(ldq=128, ldk=128, ldv=128, ldo=128, H=3), "64 * H")
        refused(L, prec, desc(ldq=-128), "64 * H")
    # the blocked output's k-steps per 32-row block are ldo / 16
    refused(L, own16(flavour), desc(o_blocked=1, ldo=96), "64 * H")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_a_relative_position_table_narrower_than_the_heads(flavour):
    L = hip.lib(flavour)
    for prec, _ in layouts(flavour):
        refused(L, prec, desc(rel_pos=P, rel_u=P, rel_v=P, rel_R=4, ld_pos=96), "ld_pos")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_blocked_windows_outside_their_matrix(flavour):
    L = hip.lib(flavour)
    prec = own16(flavour)
    refused(L, prec, desc(Q=P, q_blocked=1, q_col=32, q_n=128), "inside its q_n / kv_n")
    refused(L, prec, desc(q_blocked=1, q_col=256, q_n=256), "inside")
    refused(L, prec, desc(kv_blocked=1, k_col=0, v_col=160, kv_n=256), "inside")
    refused(L, prec, desc(kv_blocked=1, k_col=192, v_col=0, kv_n=256), "inside")
    refused(L, prec, desc(kv_blocked=1, k_col=4, v_col=128, kv_n=256), "col % 8")
    refused(L, prec, desc(kv_blocked=1, k_col=-8, v_col=128, kv_n=256), "col >= 0")
    refused(L, prec, desc(q_blocked=1, q_col=-64, q_n=128), "col >= 0")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_the_existing_bad_geometries(flavour):
    L = hip.lib(flavour)
    b16 = own16(flavour)
    rel = dict(rel_pos=P, rel_u=P, rel_v=P, rel_R=4, ld_pos=128)
    # rows 16-byte aligned
    refused(L, b16, desc(ldq=132), "16-byte")
    refused(L, b16, desc(ldo=140), "16-byte")
    # blocked operands: 16-bit layouts, no relative positions, column counts % 32 == 0 (the blocked output: ldo)
    refused(L, b16, desc(q_blocked=1, q_n=144), "% 32")
    refused(L, b16, desc(kv_blocked=1, k_col=0, v_col=128, kv_n=272), "% 32")
    refused(L, b16, desc(o_blocked=1, ldo=136), "% 32")
    refused(L, b16, desc(q_blocked=1, q_n=128, **rel), "without relative positions")
    # relative positions: self attention, 0 <= R <= 31, u and v
    refused(L, b16, desc(Lk=11, **rel), "self attention")
    refused(L, b16, desc(**dict(rel, rel_R=32)), "<= 31")
    refused(L, b16, desc(**dict(rel, rel_R=-1)), "<= 31")
    refused(L, b16, desc(**dict(rel, rel_u=None)), "relative positions")
    refused(L, b16, desc(**dict(rel, rel_v=None)), "relative positions")
    refused(L, b16, None, "null descriptor")
    if flavour == "f16":  # the half-precision build holds the 16-bit layout only
        refused(L, hip.PRECISION["fp32"], desc(), "CN_PRECISION_F16")
        refused(L, hip.PRECISION["bf16"], desc(), "CN_PRECISION_F16")
        return
    f32, x3 = hip.PRECISION["fp32"], hip.PRECISION["bf16x3"]
    refused(L, hip.PRECISION["fp16"], desc(), "libcassnat_hip_f16")
    refused(L, f32, desc(ldk=130), "16-byte")
    refused(L, x3, desc(ldq=144), "multiples of 32")
    refused(L, x3, desc(ldo=160 + 16), "multiples of 32")
    for prec in (f32, x3):
        refused(L, prec, desc(q_blocked=1, q_n=128), "bf16 kernels")
        refused(L, prec, desc(kv_blocked=1, k_col=0, v_col=128, kv_n=256), "bf16 kernels")
        refused(L, prec, desc(o_blocked=1, ldo=128), "bf16 kernels")
        refused(L, prec, desc(Lq=12, **rel), "self attention")
        refused(L, prec, desc(**dict(rel, rel_R=40)), "<= 31")
