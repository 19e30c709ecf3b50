"""Operand layouts of the four attention layouts and a float64 model of the fused attention kernel (csrc/attention.hip) with a
per-element error bound.  Shared by the kernel tests (test_gpu_attention.py, test_gpu_ast_kernels.py) and the CPU test that shows
the bounds are tight enough to catch the mistakes a kernel could make (test_attention_model.py).

The model states the reference's semantics (src/models/modules/attention.py): scores q . k * scale, masked keys take the
float32-min fill (a row without an allowed key averages), and RelMultiHeadedAttention.forward's relative scores with its zero-pad /
view shift, masked probabilities re-zeroed.  On top of that, the kernel's options: kcap (keys past an entry's own count are absent:
-inf), kv_mod / kv_index (which entry's keys a query set reads), and the roundings the kernel applies as part of the operation
(q + u rounded to the operand type on REL; P rounded to the operand before P . V, which the bound covers)."""
import numpy as np
import torch

EPS = 2.0 ** -24  # float32 unit roundoff
NEG_FILL = float(np.finfo(np.float32).min)  # masked attention score (the reference's masked_fill value)

LAYOUTS = {  # name: (library flavour, CN_PRECISION_*, operand name the library must report)
    "fp32": (None, 0, "bf16"),
    "bf16": (None, 1, "bf16"),
    "fp16": ("f16", 4, "fp16"),
    "bf16x3": (None, 3, "bf16"),
}


def gamma(n):
    return n * EPS / (1 - n * EPS)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def to_layout(x, layout, device="cuda"):
    """float32 tensor (rows of C columns) -> (tensor in the layout's element bytes on ``device``, float64 operand the kernel
    sees).  Split-bf16 rows: per group of 32 elements [32 bf16 hi][32 bf16 lo]."""
    if layout == "fp32":
        return x.to(device), x.double()
    if layout in ("bf16", "fp16"):
        h = x.to(torch.bfloat16 if layout == "bf16" else torch.float16)
        return h.to(device), h.double()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    sh = x.shape[:-1] + (x.shape[-1] // 32, 1, 32)
    packed = torch.cat([hi.reshape(sh), lo.reshape(sh)], dim=-2).reshape(x.shape[:-1] + (2 * x.shape[-1],))
    return packed.to(device), hi.double() + lo.double()


def from_layout(t, layout):
    if layout != "bf16x3":
        return t.cpu().double()
    c = t.shape[-1] // 2
    g = t.cpu().reshape(t.shape[:-1] + (c // 32, 2, 32))
    return (g[..., 0, :].double() + g[..., 1, :].double()).reshape(t.shape[:-1] + (c,))


def out_ulp(ref, layout):
    """One ulp of the output element at |ref| (split-bf16: the bound of its hi + lo rounding, ~17 significant bits)."""
    sp = torch.from_numpy(ulp32(ref.numpy()))  # float32 ulp: 2^(e - 23)
    if layout == "fp32":
        return torch.zeros_like(ref)
    if layout == "bf16x3":
        return ref.abs() * 2.0 ** -16 + 1e-38
    if layout == "bf16":
        return sp * 2.0 ** 16
    return torch.clamp(sp * 2.0 ** 13, min=2.0 ** -24)


def round_operand(x32, layout):
    """float32 tensor -> float64 value after the kernel's conversion to the layout's operand (split-bf16: hi + lo)."""
    if layout == "fp32":
        return x32.double()
    if layout in ("bf16", "fp16"):
        return x32.to(torch.bfloat16 if layout == "bf16" else torch.float16).double()
    hi = x32.to(torch.bfloat16)
    return hi.double() + (x32 - hi.float()).to(torch.bfloat16).double()


# relative error of P as the P . V product sees it (rounded to the operand; split-bf16: hi + lo and the dropped lo . lo term), the
# absolute error of a half-precision subnormal probability, and the split-bf16 score product's dropped lo . lo term
P_ROUND = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -15}
P_SUB = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25, "bf16x3": 0.0}
S_SPLIT = {"fp32": 0.0, "bf16": 0.0, "fp16": 0.0, "bf16x3": 2.0 ** -16}

MISTAKES = ("rel_sign", "rel_clamp_lo", "rel_clamp_hi", "rel_uv_swap", "rel_bd_unscaled", "rel_masked_average", "plain_masked_zero",
            "kcap_fill", "iv_inclusive", "causal_strict", "klen_ignored")


def attention_model(q, k, v, scale, layout, keymask=None, klen=None, kcap=None, kv_of=None, intervals=None, causal=False,
                    rel=None, mistakes=()):
    """float64 attention of B query sets over E key / value entries -> (out, bound), both (B, Lq, 64 H).

    q (B, Lq, 64 H), k / v (E, Lk, 64 H): float64 operands as the kernel sees them.  kv_of (B,): the entry query set b reads (its
    K, V, keymask and kcap; default b).  keymask (E, Lk) bool; klen (B,); kcap (E,): keys j >= kcap[e] of entry e are absent;
    intervals (B, Lq, 4) (s1, e1, s2, e2): key j allowed for row i iff j in [s1, e1) or [s2, e2); causal: j <= i.
    rel: dict(pos=(2R+1, 64 H) float64 of the fp32 table, u, v=(64 H,) float32 tensors, R) - relative-position self attention.
    ``mistakes``: names from MISTAKES, each a deliberate error (only to show that the bounds would catch it)."""
    B, Lq, d = q.shape
    E, Lk, _ = k.shape
    H = d // 64
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    kv_of = torch.arange(B) if kv_of is None else torch.as_tensor(kv_of).long()
    jj, ii = torch.arange(Lk), torch.arange(Lq)
    allowed = torch.ones(B, Lq, Lk, dtype=torch.bool)
    if keymask is not None:
        allowed &= torch.as_tensor(keymask).bool()[kv_of][:, None, :]
    if klen is not None and "klen_ignored" not in bad:
        allowed &= jj[None, None, :] < torch.as_tensor(klen).long()[:, None, None]
    if intervals is not None:
        iv = torch.as_tensor(intervals).long()
        end = (lambda j, e: j <= e) if "iv_inclusive" in bad else (lambda j, e: j < e)
        j3 = jj[None, None, :]
        allowed &= ((j3 >= iv[..., 0:1]) & end(j3, iv[..., 1:2])) | ((j3 >= iv[..., 2:3]) & end(j3, iv[..., 3:4]))
    if causal:
        allowed &= (jj[None, :] < ii[:, None]) if "causal_strict" in bad else (jj[None, :] <= ii[:, None])
    present = torch.ones(B, Lk, dtype=torch.bool)
    if kcap is not None:
        present = jj[None, :] < torch.as_tensor(kcap).long()[kv_of][:, None]

    def heads(x):
        return x.reshape(x.shape[0], x.shape[1], H, 64).transpose(1, 2)

    Kh, Vh = heads(k)[kv_of], heads(v)[kv_of]  # (B, H, Lk, 64)
    if rel is None:
        qh = heads(q)
        s = qh @ Kh.transpose(-1, -2) * scale
        a = qh.abs() @ Kh.abs().transpose(-1, -2) * scale
    else:
        assert Lq == Lk and kcap is None
        R = rel["R"]
        u32, v32 = (rel["v"], rel["u"]) if "rel_uv_swap" in bad else (rel["u"], rel["v"])
        q32 = q.float()  # (the operand values are float32 numbers)
        qu = round_operand(q32 + u32, layout)  # the kernel's query operand: q + u rounded to the layout
        qv = (q32 + v32).double()  # (q + v) . P stays in float32 arithmetic
        # RelPositionalEncoding: the 2 Lq - 1 rows of distances -(Lq - 1) .. Lq - 1, clamped to [-R, R]
        table, centre, clamp = rel["pos"], R, R
        if "rel_clamp_lo" in bad:
            clamp = R - 1
        if "rel_clamp_hi" in bad:  # (reads one row past either end of the table: zeros here)
            table, centre, clamp = torch.cat([torch.zeros(1, d, dtype=table.dtype), table, torch.zeros(1, d, dtype=table.dtype)]), R + 1, R + 1
        dist = torch.arange(-(Lq - 1), Lq)
        if "rel_sign" in bad:
            dist = -dist
        pos = table[torch.clamp(dist, -clamp, clamp) + centre].reshape(2 * Lq - 1, H, 64).transpose(0, 1)  # (H, 2 Lq - 1, 64)

        def shift(bd):  # attention.py:124-128, literally
            zero = torch.zeros(*bd.shape[:3], 1, dtype=bd.dtype)
            padded = torch.cat([zero, bd], dim=-1).view(*bd.shape[:2], bd.shape[3] + 1, bd.shape[2])
            return padded[:, :, 1:].reshape(bd.shape)[:, :, :, :Lq]

        quh, qvh = heads(qu), heads(qv)
        ac = quh @ Kh.transpose(-1, -2)
        bd = shift(qvh @ pos.transpose(-1, -2)[None])
        s = ac * scale + bd if "rel_bd_unscaled" in bad else (ac + bd) * scale
        a = (quh.abs() @ Kh.abs().transpose(-1, -2) + shift(qvh.abs() @ pos.abs().transpose(-1, -2)[None])) * scale
    al = allowed[:, None]
    pr = present[:, None, None, :]
    sm = torch.where(al, s, torch.full_like(s, NEG_FILL))
    sm = torch.where(pr, sm, torch.full_like(s, NEG_FILL if "kcap_fill" in bad else -np.inf))
    p = torch.softmax(sm, dim=-1)
    none_allowed = ~al.any(-1, keepdim=True)
    if rel is not None and "rel_masked_average" not in bad:
        p = p.masked_fill(~al, 0.0)  # softmax(...).masked_fill(mask == 0, 0) (attention.py:133-134)
    if rel is None and "plain_masked_zero" in bad:
        p = p.masked_fill(none_allowed, 0.0)
    out = p @ Vh
    # fp32 accumulation: 64-term score sums (+ REL's (q + v) . P term and the addition), the scale, exp; the sequential key sums of
    # the numerator and of the normaliser; P rounded to the operand; the final multiply
    ds = torch.where(al & pr, gamma(66) * a + S_SPLIT[layout] * a + 2 * EPS * s.abs(), torch.zeros_like(s)).amax(-1, keepdim=True)
    ds = ds + 4 * EPS
    mass = p @ Vh.abs()
    nk = present.sum(-1).double()[:, None, None, None]
    sub = (present[:, None, None, :].double() @ Vh.abs()) * P_SUB[layout]
    bound = 2 * (2 * ds * (mass + out.abs()) + gamma(nk + 2) * (mass + out.abs()) + 2 * EPS * out.abs())
    bound = bound + P_ROUND[layout] * mass + sub
    if rel is not None:
        bound = torch.where(none_allowed, torch.zeros_like(bound), bound)  # (exactly 0)

    def merge(x):
        return x.transpose(1, 2).reshape(B, Lq, d)

    out, bound = merge(out), merge(bound)
    half_ulp = out_ulp(out.abs() + bound, layout) * (1.0 if layout == "bf16x3" else 0.5)
    return out, bound + half_ulp


# ============================================================================================ seeded cases (host tensors only)
def form_of(layout, B, H, Lq, Lk, rel=False):
    """The launch form run_attention (attention.hip) picks for this shape: the library reads no switch, the shape decides."""
    if rel:
        return "staged2-rel"
    if layout in ("bf16", "fp16") and Lk <= 256:
        return "res8" if Lq > 128 else ("res4" if Lq > 64 else "res2")
    return "staged4" if -(-Lq // 128) * H * B >= 1024 else "staged2"


def key_masks(E, Lk, g):
    """keymask (E, Lk): entry 0 all valid (its tiles take the plain / cut paths), entry 1 holes and a padded tail, entry 2 nothing
    valid, later entries holes."""
    km = torch.rand(E, Lk, generator=g) > 0.25
    km[0] = True
    if E > 1:
        km[1, max(1, Lk - Lk // 3):] = False
    if E > 2:
        km[2] = False
    return km


def row_intervals(B, Lq, Lk, g):
    """(B, Lq, 4) (s1, e1, s2, e2): two intervals, single frames, empty rows, whole rows."""
    s = torch.randint(0, Lk, (B, Lq, 4), generator=g)
    iv = torch.stack([s[..., 0], s[..., 0] + 1 + s[..., 1] % 9, s[..., 2], s[..., 2] + 1 + s[..., 3] % 5], -1)
    kind = torch.arange(Lq)[None, :].expand(B, Lq) % 5
    one = iv[..., 0][kind == 1]
    iv[kind == 1] = torch.stack([one, one + 1, torch.zeros_like(one), torch.zeros_like(one)], -1)  # one frame, second interval empty
    iv[kind == 2] = torch.tensor([3, 3, 0, 0])  # empty: no allowed key (a uniform average)
    iv[kind == 3] = torch.tensor([0, Lk, 0, 0])  # the whole row
    return torch.clamp(iv, 0, Lk).int()


def make_case(B, H, Lq, Lk, seed, masks="plain", E=None, kv_mod=0, kv_index=None, kcap=None, rel_R=None, scale=0.125, qgain=1.0,
              kgain=None):
    """Inputs of one launch: float32 q (B, Lq, 64 H), k / v (E, Lk, 64 H) and the mask sources of ``masks`` (a "+"-joined subset
    of keymask, klen, iv, causal).  kv_mod > 0 / kv_index (B,): query set b reads entry b % kv_mod / kv_index[b].  kcap (E,).
    kgain (Lk,): a per-key factor on K (online-softmax cases)."""
    g = torch.Generator().manual_seed(seed)
    d = 64 * H
    E = B if E is None else E
    kv_of = None
    if kv_mod:
        kv_of = torch.arange(B) % kv_mod
    if kv_index is not None:
        kv_index = torch.as_tensor(kv_index, dtype=torch.int32)
        kv_of = kv_index.long()
    if kcap is not None:
        kcap = torch.as_tensor(kcap, dtype=torch.int32)
    c = dict(B=B, H=H, Lq=Lq, Lk=Lk, E=E, scale=scale, kv_mod=kv_mod, kv_index=kv_index, kv_of=kv_of, kcap=kcap, keymask=None, klen=None, intervals=None,
             causal=False, rel=None)
    c["q"] = torch.randn(B, Lq, d, generator=g) * qgain
    c["k"] = torch.randn(E, Lk, d, generator=g)
    c["v"] = torch.randn(E, Lk, d, generator=g)
    if kgain is not None:
        c["k"] = c["k"] * kgain[None, :, None]
    parts = set(masks.split("+")) - {"plain"}
    if "keymask" in parts:
        c["keymask"] = key_masks(E, Lk, g)
    if "klen" in parts:  # Lk on query set 0 (plain tiles), an inner length, 0, Lk - 1
        c["klen"] = torch.tensor([(Lk, max(1, Lk // 2 + 3), 0, Lk - 1)[b % 4] for b in range(B)], dtype=torch.int32)
    if "iv" in parts:
        c["intervals"] = row_intervals(B, Lq, Lk, g)
    c["causal"] = "causal" in parts
    if rel_R is not None:
        ld_pos = d + 32
        pos = torch.randn(2 * rel_R + 1, ld_pos, generator=g) * 0.5
        pos[:, d:] = float("nan")  # (columns past the heads: never read)
        c["rel"] = dict(R=rel_R, pos=pos, ld_pos=ld_pos, u=torch.randn(d, generator=g) * 0.5, v=torch.randn(d, generator=g) * 0.5)
    return c


def model_of(c, layout, q64, k64, v64, mistakes=(), rows=None):
    """attention_model of case ``c`` for the layout's operands; ``rows``: only these query sets (a sample of a large launch)."""
    sel = torch.arange(c["B"]) if rows is None else torch.as_tensor(rows)
    kv_of = sel if c["kv_of"] is None else torch.as_tensor(c["kv_of"]).long()[sel]
    rel = None
    if c["rel"] is not None:
        r = c["rel"]
        rel = dict(R=r["R"], pos=r["pos"][:, :64 * c["H"]].double(), u=r["u"], v=r["v"])
    pick = (lambda t: None if t is None else torch.as_tensor(t)[sel])
    return attention_model(q64[sel], k64, v64, c["scale"], layout, keymask=c["keymask"], klen=pick(c["klen"]), kcap=c["kcap"],
                           kv_of=kv_of, intervals=pick(c["intervals"]), causal=c["causal"], rel=rel, mistakes=mistakes)


def operands(c, layout):
    """float64 q / k / v as the kernel sees them in ``layout`` (host only)."""
    return tuple(to_layout(c[n], layout, device="cpu")[1] for n in ("q", "k", "v"))
