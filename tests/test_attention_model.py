"""The float64 attention model's bounds can fail (no device needed): at the shapes the GPU tests use (test_gpu_attention.py), each
mistake below moves some output element by more than the bf16 bound - the loosest of the four layouts - so the GPU gates would
catch a kernel that made it."""
import pytest
import torch

from attention_model import make_case, model_of, operands


def overshoot(c, mistakes=(), **changed):
    """max over elements of |wrong - right| - bf16 bound (> 0: the mistake is caught)."""
    q, k, v = operands(c, "bf16")
    ref, bound = model_of(c, "bf16", q, k, v)
    wrong, _ = model_of(dict(c, **changed), "bf16", q, k, v, mistakes=mistakes)
    return float(((wrong - ref).abs() - bound).max())


def rel_case():  # test_relative_positions R8-L65-H8
    return make_case(3, 8, 65, 65, seed=8 * 7 + 65, masks="keymask+klen", rel_R=8)


def kcap_case():  # test_kcap, Lk 256, keymask + klen: entry 0's own keys all masked
    c = make_case(4, 4, 256, 256, seed=256 + len("keymask+klen"), masks="keymask+klen", kcap=[37, 1, 256, 200])
    c["keymask"][0, :] = False
    c["keymask"][3, :] = True
    return c


CASES = {
    "rel_sign": rel_case,
    "rel_clamp_lo": rel_case,
    "rel_clamp_hi": rel_case,
    "rel_uv_swap": rel_case,
    "rel_bd_unscaled": rel_case,
    "rel_masked_average": rel_case,
    "plain_masked_zero": lambda: make_case(4, 4, 127, 64, seed=0, masks="keymask+klen"),
    "kcap_fill": kcap_case,
    "iv_inclusive": lambda: make_case(2, 1, 256, 129, seed=0, masks="keymask+klen+iv"),
    "causal_strict": lambda: make_case(3, 1, 300, 300, seed=0, masks="keymask+causal"),
    "klen_ignored": lambda: make_case(4, 4, 127, 64, seed=0, masks="keymask+klen"),
}


@pytest.mark.parametrize("mistake", list(CASES))
def test_bf16_bound_catches(mistake):
    assert overshoot(CASES[mistake](), mistakes=(mistake,)) > 0


def test_bf16_bound_catches_kv_mod_read_as_blocks():
    """kv_mod: query set b reads entry b % kv_mod, not b // (B / kv_mod) (test_kv_mod's ESA shape: 3 sets of 2 utterances)."""
    c = make_case(6, 4, 33, 129, seed=7, masks="keymask+klen+iv", E=2, kv_mod=2)
    assert overshoot(c, kv_of=torch.arange(6) // 3) > 0


@pytest.mark.parametrize("layout", ["fp32", "bf16", "fp16", "bf16x3"])
def test_model_matches_the_reference_forms(layout):
    """Sanity of the model itself: without masks its REL scores equal the closed form clamp(j - i) of the relative table (the
    reference's shift selects column j - i + Lq - 1), and a plain row is softmax(q k^T * scale) v."""
    c = make_case(2, 4, 40, 40, seed=3, rel_R=5)
    q, k, v = operands(c, layout)
    out, bound = model_of(c, layout, q, k, v)
    r = c["rel"]
    H, L = 4, 40
    qu = (q.float() + r["u"]).to({"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "bf16x3": torch.float32}[layout])
    if layout == "bf16x3":  # (hi + lo of q + u)
        hi = qu.to(torch.bfloat16)
        qu = hi.double() + (qu - hi.float()).to(torch.bfloat16).double()
    qu, qv = qu.double(), (q.float() + r["v"]).double()
    dist = torch.arange(L)[None, :] - torch.arange(L)[:, None]
    P = r["pos"][:, :256].double()[torch.clamp(dist, -5, 5) + 5]  # (L, L, d)
    hd = lambda x: x.reshape(*x.shape[:-1], H, 64)  # noqa: E731
    s = (torch.einsum("bihc,bjhc->bhij", hd(qu), hd(k)) + torch.einsum("bihc,ijhc->bhij", hd(qv), hd(P))) * 0.125
    want = torch.einsum("bhij,bjhc->bihc", torch.softmax(s, -1), hd(v)).reshape(2, L, 256)
    assert torch.allclose(out, want, rtol=0, atol=1e-12)
    assert (bound > 0).all()
