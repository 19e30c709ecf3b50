"""The fused attention kernel (csrc/attention.hip) in every launch form, against the float64 model of attention_model.py and bit for
bit against itself where merged passes and the layouts rely on it.

Every launch goes through cn_op_attention_desc, which reaches all of AttnArgs.  The form is chosen by the shape alone (the product
library reads no switch): RES (bf16 / fp16, Lk <= 256: all keys resident in LDS) with 8 / 4 / 2 waves by Lq, the staged form
with 4 waves (B * H * ceil(Lq / 128) >= 1024) or 2, and the relative-position form.  Each form meets its three tile paths: plain
(no masked key), cut (a 32-key sub-tile straddles kcap or Lk) and full mask.  Rows are wider than the data (as production's fused
[M][3d] Q|K|V buffer), their spare columns hold NaN and the output's spare columns a sentinel that must survive.

Run with -s to see the worst error / bound ratio per layout and form."""
import ctypes as C

import numpy as np
import pytest
import torch

from attention_model import LAYOUTS, form_of, from_layout, make_case, model_of, operands, to_layout
from cassnat_asr_public_amd import hip

pytestmark = pytest.mark.gpu

ES = {"fp32": 4, "bf16": 2, "fp16": 2, "bf16x3": 4}  # bytes per element as the kernel counts them (split-bf16: hi + lo)
PAD = 32  # spare columns of every row-major operand
SENTINEL = 7.0
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |out - fp64| / bound per layout and form:")
    for (layout, form), (ratio, err) in sorted(WORST.items()):
        print(f"  {layout:7s} {form:12s} {ratio:.3f}  (|err| {err:.2e})")


def stream():
    return hip.current_stream()


def ptr(t, layout=None, col=0):
    return None if t is None else t.data_ptr() + col * (ES[layout] if layout else 0)


def lib_of(layout):
    flavour, prec, operand = LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    return L, prec


def blk16_off(m, c, N):
    """cn_blk16_off (common.h): byte offset of the 16-byte chunk at (row m, column c % 8 == 0) of a blocked [M][N] matrix."""
    return ((((m >> 5) * (N >> 5) + (c >> 5)) << 1) + ((c >> 4) & 1)) * 1024 + ((((c >> 3) & 1) << 5) + (m & 31)) * 16


def oblk_off(m, c, ldo):
    """The o_blocked order (AttnArgs): byte offset of the chunk at (row m, channel c % 8 == 0)."""
    return ((m >> 5) * (ldo // 16) + (c >> 4)) * 1024 + (((c >> 3) & 1) * 32 + (m & 31)) * 16


def blocked_index(M, N, off):
    """(M, N) element index into the flat blocked buffer of ceil(M / 32) * 32 rows."""
    m = np.arange(M)[:, None]
    c = np.arange(N)[None, :]
    return torch.from_numpy(off(m, c - c % 8, N) // 2 + c % 8)


def pack_blocked(x16, N):
    """Row-major 16-bit (M, N) -> the blocked buffer (rows past M: NaN)."""
    M = x16.shape[0]
    buf = torch.full((-(-M // 32) * 32 * N,), NAN, dtype=x16.dtype)
    buf[blocked_index(M, N, blk16_off).reshape(-1)] = x16.reshape(-1)
    return buf


def attend(layout, c, blocked=None):
    """Launch case ``c``; returns (output float64 (B, Lq, 64 H), raw output rows (B * Lq, 64 H) of the layout's bits).

    blocked: None (row-major), "self" (production's encoder self attention: one blocked [M][3d] Q|K|V matrix, blocked output) or
    "src" (decoder source attention: Q blocked [M][d], K|V a kv_slot window of a wider blocked matrix, blocked output)."""
    L, prec = lib_of(layout)
    B, H, Lq, Lk, E = c["B"], c["H"], c["Lq"], c["Lk"], c["E"]
    d = 64 * H
    q, k, v = c["q"].reshape(B * Lq, d), c["k"].reshape(E * Lk, d), c["v"].reshape(E * Lk, d)
    f = dict(B=B, H=H, Lq=Lq, Lk=Lk, scale=c["scale"], kcap_stride=1)
    keep = []
    fused = c["kv_of"] is None and B == E and Lq == Lk
    if blocked is None:
        if fused:
            X = torch.full((B * Lq, 3 * d + PAD), NAN)
            X[:, :d], X[:, d:2 * d], X[:, 2 * d:3 * d] = q, k, v
            Xd = to_layout(X, layout)[0]
            f.update(Q=ptr(Xd), K=ptr(Xd, layout, d), V=ptr(Xd, layout, 2 * d), ldq=3 * d + PAD, ldk=3 * d + PAD, ldv=3 * d + PAD)
            keep.append(Xd)
        else:
            Qx = torch.full((B * Lq, d + PAD), NAN)
            Qx[:, :d] = q
            KV = torch.full((E * Lk, 2 * d + PAD), NAN)
            KV[:, :d], KV[:, d:2 * d] = k, v
            Qd, KVd = to_layout(Qx, layout)[0], to_layout(KV, layout)[0]
            f.update(Q=ptr(Qd), K=ptr(KVd), V=ptr(KVd, layout, d), ldq=d + PAD, ldk=2 * d + PAD, ldv=2 * d + PAD)
            keep += [Qd, KVd]
        ldo = d + PAD
        O = to_layout(torch.full((B * Lq, ldo), SENTINEL), layout)[0]
    else:
        dt = torch.bfloat16 if layout == "bf16" else torch.float16
        if blocked == "self":
            assert fused
            Xd = pack_blocked(torch.cat([q, k, v], 1).to(dt), 3 * d).cuda()
            f.update(Q=ptr(Xd), K=ptr(Xd), V=ptr(Xd), q_blocked=1, kv_blocked=1, q_col=0, k_col=d, v_col=2 * d, q_n=3 * d,
                     kv_n=3 * d, ldq=3 * d, ldk=3 * d, ldv=3 * d)
            keep.append(Xd)
            ldo = d
        else:
            kv_cols = 3 * 2 * d  # three layers' K|V; this one is slot 1
            KV = torch.full((E * Lk, kv_cols), NAN)
            KV[:, 2 * d:3 * d], KV[:, 3 * d:4 * d] = k, v
            Qd, KVd = pack_blocked(q.to(dt), d).cuda(), pack_blocked(KV.to(dt), kv_cols).cuda()
            f.update(Q=ptr(Qd), K=ptr(KVd), V=ptr(KVd), q_blocked=1, kv_blocked=1, q_col=0, k_col=2 * d, v_col=3 * d, q_n=d,
                     kv_n=kv_cols, ldq=d, ldk=kv_cols, ldv=kv_cols)
            keep += [Qd, KVd]
            ldo = d + 64  # (spare channels: must stay untouched)
        O = torch.full((-(-B * Lq // 32) * 32 * ldo,), SENTINEL, dtype=dt).cuda()
        f.update(o_blocked=1)
    f.update(O=ptr(O), ldo=ldo)
    if c["keymask"] is not None:
        km = c["keymask"].to(torch.uint8).cuda()
        f.update(keymask=ptr(km))
        keep.append(km)
    if c["klen"] is not None:
        kl = c["klen"].cuda()
        f.update(klen=ptr(kl))
        keep.append(kl)
    if c["kcap"] is not None:  # every third int: the rest of a UttMeta record
        kc = torch.full((E, 3), -99, dtype=torch.int32)
        kc[:, 0] = c["kcap"]
        kc = kc.cuda()
        f.update(kcap=ptr(kc), kcap_stride=3)
        keep.append(kc)
    if c["kv_mod"]:
        f.update(kv_mod=c["kv_mod"])
    if c["kv_index"] is not None:
        ki = c["kv_index"].cuda()
        f.update(kv_index=ptr(ki))
        keep.append(ki)
    if c["intervals"] is not None:  # [B][Lq + 1][4]: a spare row, as production's Tp + 1
        iv = torch.full((B, Lq + 1, 4), -5, dtype=torch.int32)
        iv[:, :Lq] = c["intervals"]
        iv = iv.cuda()
        f.update(intervals=ptr(iv), iv_stride=Lq + 1)
        keep.append(iv)
    f.update(causal=int(c["causal"]))
    if c["rel"] is not None:
        r = c["rel"]
        pos, u, vv = r["pos"].cuda(), r["u"].cuda(), r["v"].cuda()
        f.update(rel_pos=ptr(pos), rel_u=ptr(u), rel_v=ptr(vv), rel_R=r["R"], ld_pos=r["ld_pos"])
        keep += [pos, u, vv]
    desc = hip.CnAttnDesc(**f)
    hip.check(L.cn_op_attention_desc(prec, C.byref(desc), stream()), "cn_op_attention_desc", L)
    torch.cuda.synchronize()
    M = B * Lq
    if blocked is None:
        full = from_layout(O, layout)
        assert torch.equal(full[:, d:], torch.full((M, ldo - d), SENTINEL, dtype=torch.float64)), "a column past the heads was written"
        raw = O.cpu()
        raw = raw[:, :2 * d] if layout == "bf16x3" else raw[:, :d]
        got = full[:, :d]
    else:
        o = O.cpu()
        allrows = o[blocked_index(M, ldo, oblk_off)]
        assert torch.equal(allrows[:, d:].double(), torch.full((M, ldo - d), SENTINEL, dtype=torch.float64))
        raw = allrows[:, :d]
        got = raw.double()
    return got.reshape(B, Lq, d), raw


def bits(raw):
    return raw.contiguous().view(torch.int16 if raw.element_size() == 2 else torch.int32)


def check_model(layout, c, got, what, rows=None):
    """|got - model| <= bound on every element (of the sampled query sets ``rows``); records the worst ratio of the form."""
    assert torch.isfinite(got).all(), what
    q64, k64, v64 = operands(c, layout)
    ref, bound = model_of(c, layout, q64, k64, v64, rows=rows)
    g = got if rows is None else got[torch.as_tensor(rows)]
    err = (g - ref).abs()
    if not (err <= bound).all():
        bad = (err - bound).argmax()
        idx = np.unravel_index(int(bad), tuple(err.shape))
        raise AssertionError(f"{layout} {what}: |err| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e} at (b, i, c) = {idx}; "
                             f"got {float(g[idx]):.6g}, fp64 {float(ref[idx]):.6g}; {int((err > bound).sum())} elements out of bound")
    ratio = float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())
    form = form_of(layout, c["B"], c["H"], c["Lq"], c["Lk"], c["rel"] is not None)
    WORST[(layout, form)] = max(WORST.get((layout, form), (0.0, 0.0)), (ratio, float(err.max())))
    print(f"{layout} {form} {what}: worst |err| {float(err.max()):.2e} = {ratio:.3f} of the bound")
    return ref


# ============================================================================================ against the float64 model
M_ALL = "keymask+klen+iv+causal"
SHAPES = {  # form on the 16-bit layouts: [(B, H, Lq, Lk, masks), ...] - the fp32 / split-bf16 layouts run them staged
    "res8": [(3, 4, 129, 256, "plain"), (3, 4, 129, 256, "keymask+causal"), (3, 8, 255, 33, "keymask+klen"),
             (2, 1, 256, 129, "keymask+klen+iv"), (2, 1, 256, 129, M_ALL)],
    "res4": [(3, 8, 65, 255, "plain"), (3, 8, 65, 255, "keymask+klen+iv"), (4, 4, 127, 64, "keymask+klen"),
             (3, 1, 128, 1, "keymask+causal"), (4, 4, 127, 64, M_ALL)],
    "res2": [(4, 4, 1, 63, "keymask+klen"), (3, 8, 33, 31, "plain"), (3, 8, 33, 31, "keymask+klen+iv"),
             (3, 1, 64, 65, "keymask+causal"), (4, 4, 63, 127, M_ALL)],
    "staged2": [(3, 4, 33, 257, "plain"), (3, 4, 33, 257, "keymask+klen"), (2, 8, 129, 511, "keymask+klen+iv"),
                (3, 1, 300, 300, "keymask+causal"), (3, 1, 300, 300, M_ALL)],
    "staged4": [(43, 8, 300, 300, "keymask+klen"), (43, 8, 300, 300, M_ALL)],
}
LAYOUT_NAMES = list(LAYOUTS)


def cases_for(shapes):
    out = []
    for layout in LAYOUT_NAMES:
        for i, (B, H, Lq, Lk, masks) in enumerate(shapes):
            form = form_of(layout, B, H, Lq, Lk)
            out.append(pytest.param(layout, (B, H, Lq, Lk, masks), i, id=f"{layout}-{form}-{masks}-{B}x{H}x{Lq}x{Lk}"))
    return out


@pytest.mark.parametrize("layout,shape,seed", cases_for([s for v in SHAPES.values() for s in v]))
def test_masks_in_every_form(layout, shape, seed):
    """Key padding with holes, klen (Lk, 0, inner), intervals (two, single frames, empty rows, whole rows), causal, combined."""
    B, H, Lq, Lk, masks = shape
    c = make_case(B, H, Lq, Lk, seed=100 + seed + Lq + Lk, masks=masks)
    form = form_of(layout, B, H, Lq, Lk)
    if layout in ("bf16", "fp16"):  # the shape list covers every form of the 16-bit layouts on purpose
        assert any(shape in v and f == form for f, v in SHAPES.items())
    got, _ = attend(layout, c)
    rows = [0, 1, 2, B - 1] if B > 8 else None  # (the staged 4-wave grid: a sample of the 43 query sets for the model)
    check_model(layout, c, got, masks, rows=rows)


KCAP_CASES = [  # (Lk, kcap per entry): not a multiple of 32, 1, Lk, ...; RES on the 16-bit layouts for Lk <= 256
    (256, [37, 1, 256, 200]),
    (300, [37, 1, 300, 257]),
]


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("Lk,kcap", KCAP_CASES)
@pytest.mark.parametrize("masks", ["plain", "keymask+klen"])
def test_kcap(layout, Lk, kcap, masks):
    """Keys past an entry's kcap are absent (-inf): alone the cut path, with a keymask the full mask path; entry 0's own keys are
    all masked, so its rows average over its kcap keys (not over Lk)."""
    c = make_case(4, 4, Lk, Lk, seed=Lk + len(masks), masks=masks, kcap=kcap)
    if c["keymask"] is not None:
        c["keymask"][0, :] = False  # (kcap 37: its rows average over 37 keys)
        c["keymask"][3, :] = True  # (kcap 200 / 257 < Lk with every own key valid: cut tiles inside the full mask launch)
    got, _ = attend(layout, c)
    check_model(layout, c, got, f"kcap {kcap} {masks}")


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("kcap", [None, [129, 61]])
def test_kv_mod(layout, kcap):
    """ESA sample groups: 3 query sets per utterance read entry b % 2 (K, V, keymask, kcap); intervals and klen stay per set."""
    c = make_case(6, 4, 33, 129, seed=7, masks="keymask+klen+iv", E=2, kv_mod=2, kcap=kcap)
    got, _ = attend(layout, c)
    check_model(layout, c, got, f"kv_mod 2 kcap {kcap}")


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("Lk", [200, 300])
def test_kv_index(layout, Lk):
    """AST source attention: hundreds of single-query rows, each naming its utterance (keymask per utterance)."""
    n = 300
    utt = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(Lk)).int()
    utt[:3] = torch.tensor([2, 0, 1], dtype=torch.int32)
    c = make_case(n, 4, 1, Lk, seed=Lk, masks="keymask", E=3, kv_index=utt)
    got, _ = attend(layout, c)
    check_model(layout, c, got, f"kv_index n {n}")


REL_CASES = [(20, 250, 4), (8, 65, 8), (31, 64, 4), (0, 63, 8), (1, 9, 4), (20, 9, 4), (8, 1, 8), (31, 2, 4)]


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("R,L_,H", REL_CASES, ids=[f"R{R}-L{L_}-H{H}" for R, L_, H in REL_CASES])
def test_relative_positions(layout, R, L_, H):
    """RelMultiHeadedAttention: ld_pos > 64 H, non-zero u and v, keymask with klen; entry 2 has no valid key: its rows are 0."""
    c = make_case(3, H, L_, L_, seed=R * 7 + L_, masks="keymask+klen", rel_R=R)
    got, _ = attend(layout, c)
    check_model(layout, c, got, f"rel R {R}")
    assert torch.equal(got[2], torch.zeros_like(got[2]))  # (exactly 0, attention.py:133-134)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("Lk", [256, 511])
@pytest.mark.parametrize("where", ["late", "early"])
def test_online_softmax_rescaling(layout, Lk, where):
    """Large scores: the row maximum first appears in the last key tile (every earlier tile is rescaled), or sits in tile 0 with
    tiny later tiles (their probabilities underflow towards half-precision subnormals)."""
    gain = torch.ones(Lk)
    last = (Lk - 1) // 64 * 64
    if where == "late":
        gain[last:] = 4.0
    else:
        gain[:64] = 4.0
        gain[64:] = 0.05
    c = make_case(2, 4, 100, Lk, seed=Lk, masks="keymask", qgain=3.0, kgain=gain)
    c["keymask"][1] = True
    got, _ = attend(layout, c)
    check_model(layout, c, got, f"rescale {where}")


@pytest.mark.parametrize("layout", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["self", "src"])
def test_blocked_operands_against_model_and_row_major(layout, kind):
    """Blocked Q / K|V / O at production's column offsets, with kcap (a merged pass): equal to the row-major launch bit for bit."""
    if kind == "self":  # encoder self attention of a merged pass: Q|K|V thirds of one [M][3d] matrix
        c = make_case(3, 4, 150, 150, seed=5, masks="keymask", kcap=[150, 97, 33])
    else:  # source attention: a kv_slot window of the [M][kv_cols] matrix, trigger intervals
        c = make_case(3, 4, 40, 300, seed=6, masks="keymask+iv", kcap=[300, 129, 1])
    got_b, raw_b = attend(layout, c, blocked=kind)
    check_model(layout, c, got_b, f"blocked {kind}")
    _, raw_r = attend(layout, c)
    assert torch.equal(bits(raw_b), bits(raw_r))


# ============================================================================================ bit for bit, no model
def with_garbage(c, caps, seed):
    """Keys, values and query rows past each entry's own count: large finite garbage (V past kcap meets an exact 0)."""
    g = torch.Generator().manual_seed(seed)
    for e, t in enumerate(caps):
        for n in ("q", "k", "v"):
            x = c[n]
            x[e, t:] = (torch.rand(x[e, t:].shape, generator=g) - 0.5) * 6e4
    return c


def sub_case(c, e, T, Lq=None):
    """Entry e of a merged case alone: Lk = T keys (and its first Lq query rows), no kcap."""
    Lq = T if Lq is None else Lq
    s = dict(c, B=1, E=1, Lq=Lq, Lk=T, kcap=None, kv_of=None, kv_mod=0, kv_index=None)
    s["q"], s["k"], s["v"] = c["q"][e:e + 1, :Lq].clone(), c["k"][e:e + 1, :T].clone(), c["v"][e:e + 1, :T].clone()
    s["keymask"] = None if c["keymask"] is None else c["keymask"][e:e + 1, :T].clone()
    s["klen"] = None if c["klen"] is None else c["klen"][e:e + 1].clone()
    s["intervals"] = None if c["intervals"] is None else c["intervals"][e:e + 1, :Lq].clone()
    return s


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("masks", ["plain", "keymask"])
def test_merged_pass_equals_alone(layout, masks):
    """An utterance decoded alone (Lk = T <= 256: the RES form on 16-bit layouts) equals the same utterance inside a merged pass
    (Lk = 300 > 256, kcap = T: the staged form), bit for bit - the README's "per-batch results identical to separate passes"."""
    caps = [200, 300, 129, 77]
    c = with_garbage(make_case(4, 4, 300, 300, seed=11, masks=masks, kcap=caps), caps, seed=12)
    if c["keymask"] is not None:
        for e, t in enumerate(caps):
            c["keymask"][e, t:] = False  # (padding frames are masked too, as in production)
    _, raw = attend(layout, c)
    raw = raw.reshape(4, 300, -1)
    for e in (0, 2, 3):
        T = caps[e]
        _, alone = attend(layout, sub_case(c, e, T))
        assert torch.equal(bits(alone), bits(raw[e, :T])), (layout, masks, e, T)
    # source-attention shape: 40 query rows with intervals inside the utterance
    # (intervals past T: keys that do not exist alone and are absent in the merged pass)
    caps = [129, 300, 250]
    c = with_garbage(make_case(3, 4, 40, 300, seed=13, masks="keymask+iv", kcap=caps), caps, seed=14)
    _, raw = attend(layout, c)
    raw = raw.reshape(3, 40, -1)
    for e in (0, 2):
        _, alone = attend(layout, sub_case(c, e, caps[e], Lq=40))
        assert torch.equal(bits(alone), bits(raw[e])), (layout, "src", e)


@pytest.mark.parametrize("layout", ["bf16", "fp16"])
def test_res_wave_counts_agree(layout):
    """The same K / V under the 8-, 4- and 2-wave RES forms (Lq = 300, 100, 64): the first 64 query rows are equal."""
    c = make_case(2, 4, 300, 200, seed=21, masks="keymask+klen")
    outs = []
    for Lq in (300, 100, 64):
        s = dict(c, Lq=Lq, q=c["q"][:, :Lq].clone())
        assert form_of(layout, 2, 4, Lq, 200) == {300: "res8", 100: "res4", 64: "res2"}[Lq]
        got, raw = attend(layout, s)
        check_model(layout, s, got, f"waves Lq {Lq}")
        outs.append(bits(raw.reshape(2, Lq, -1)[:, :64]))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_kv_mod_equals_separate_launches(layout):
    c = make_case(6, 4, 33, 129, seed=31, masks="keymask+klen+iv", E=2, kv_mod=2, kcap=[129, 70])
    _, raw = attend(layout, c)
    raw = raw.reshape(6, 33, -1)
    for b in range(6):
        e = b % 2
        s = dict(c, B=1, E=1, kv_mod=0, kv_of=None, kcap=c["kcap"][e:e + 1], q=c["q"][b:b + 1], k=c["k"][e:e + 1],
                 v=c["v"][e:e + 1], keymask=c["keymask"][e:e + 1], klen=c["klen"][b:b + 1], intervals=c["intervals"][b:b + 1])
        _, alone = attend(layout, s)
        assert torch.equal(bits(alone), bits(raw[b])), (layout, b)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_kv_index_equals_dense(layout):
    """Rows naming their utterance (kv_index, Lq = 1) equal the dense form (one entry per utterance, its rows as queries)."""
    bw, E = 5, 3
    dense = make_case(E, 4, bw, 200, seed=41, masks="keymask")
    _, raw_d = attend(layout, dense)
    perm = torch.randperm(E * bw, generator=torch.Generator().manual_seed(42))
    utt = (perm // bw).int()
    rows = dict(dense, B=E * bw, Lq=1, kv_index=utt, kv_of=utt.long(), q=dense["q"].reshape(E * bw, 1, -1)[perm].clone())
    _, raw_i = attend(layout, rows)
    assert torch.equal(bits(raw_i), bits(raw_d[perm]))
