"""The checks of frontend_model.py would catch what a front-end kernel can get wrong - shown on the CPU, on the case list the GPU
test (test_gpu_frontend.py) runs.  A launch is stood in for by the model's EMULATION (the stage's roundings applied, float64 sums)
writing the launch's buffers through the same run_case() the GPU test uses:

* the float64 convolution is the brute-force loop's at tiny shapes, the layout maps are permutations, expand_meta is the loop's;
* the correct emulation passes every case in every library layout;
* the emulation with one deliberate mistake fails at least one case.  The table (-s) names the check that catches each mistake
  first, the case, and what the suite's earlier measure - max |got - ref| / max |ref| over the tensor, against 5e-3 at the
  tightest - reads on the same launch.

What that earlier measure would have passed, MEASURED here (the table's last column, and test_old_max_norm_on_a_dropped_conv2_tap):
not what the issue supposed.  A dropped conv2 tap is 256 of an output's 2304 products, a third of its size as an RMS, and reads
3e-1 on the old measure; a dropped conv1 tap reads 2e-1 .. 5e-1; a missing bias, a missing ReLU, transposed taps, a wrong PE row, a
wrong row split and an e4m3 scale off by one read 1e-1 .. 1: every one of them is far above the old thresholds (1.2e-2, 6e-3,
5e-3) - the old checks would have failed on them HAD A CASE REACHED THE CODE.  What they pass: the MIX planes l and q exchanged
(7e-4: the hi plane carries the value), and everything outside the value tensor, which they never look at - a border rewritten
or a row left unwritten under halo mode 2, a halo cell that is not zero, rows stored past M, a deferred store at the wrong block
(the old shapes gave every workgroup one block), the records of a merged pass (never set), frames past an utterance's own
(never NaN).  So the suite's gain is reach (launch forms, records, halo modes, grid-stride shapes) and the cells around the
values, more than sensitivity to a single tap.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import frontend_model as fm

FOUND = {}
BIG = lambda c: "gridstride" in c["name"]
conv1 = lambda c: c["kind"] == "conv1" or c.get("c1form")
form1 = lambda c: c["form"] if c["kind"] == "conv1" else c.get("c1form")

# the cases a mistake can show on
APPLIES = {
    "tap_dropped_top": lambda c: c["kind"] == "conv1",
    "tap_dropped_bottom": lambda c: c["kind"] == "conv1",
    "tap_dropped_left": lambda c: c["kind"] == "conv1",
    "tap_dropped_right": lambda c: c["kind"] == "conv1",
    "taps_transposed": lambda c: c["kind"] == "conv1" and c["T"] > 2,
    "halo_cell_nonzero": lambda c: c["kind"] == "conv1" and c["halo"] == 1,
    "border_rewritten_halo2": lambda c: c["kind"] == "conv1" and c["halo"] == 2,
    "past_own_unwritten_halo2": lambda c: conv1(c) and c["halo"] == 2 and c["subs"],
    "frames_past_read": lambda c: conv1(c) and c["subs"],
    "t1_own_from_T": lambda c: conv1(c) and c["subs"],
    "record_of_wrong_batch": lambda c: conv1(c) and c["subs"],
    "flush_at_previous_block": lambda c: form1(c) in ("f8m", "m16"),
    "rows_past_M_stored": lambda c: c["kind"] != "conv1" and (c["M"] if c["kind"] == "linear" else c["B"] * fm.sub(c["T1"]) * fm.sub(c["F1"])) % 256,
    "row_split_T1_for_T2": lambda c: c["kind"] == "conv2" and c["B"] > 1,
    "hi_lo_swapped": lambda c: (c["kind"] == "conv1" and fm.fmt1(c) in ("x3", "planes")) or (c["kind"] == "conv2" and c["form"] == "x3" and not c["c1form"]),
    "mix_l_q_swapped": lambda c: form1(c) == "mix",
    "e4m3_scale_off_by_one": lambda c: c["kind"] != "conv1" and c["form"] == "f8",
    "bias_missing": lambda c: True,
    "relu_missing": lambda c: c["kind"] != "linear",
    "pe_row_div": lambda c: c["kind"] == "linear" and c["pe"] and c["M"] > c["period"],
    "lda_ignored": lambda c: c["kind"] == "linear" and c["lda"] != c["K"] and c["M"] > 1,
}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nmistake: library, the check that catches it first, case, rms ratio of an aggregate failure, the old max-norm measure")
    for (name, layout), (kind, case, ratio, old) in sorted(FOUND.items()):
        print(f"  {name:26s} {layout:5s} {kind:10s} {case:52s} {'' if ratio is None else f'{ratio:8.1f}'}  {old}")
    fm._MODEL.clear()
    fm._W.clear()


def test_float64_convolution_is_the_loop():
    g = torch.Generator().manual_seed(1)
    for Ci, Co, H, W in ((1, 3, 1, 1), (1, 2, 2, 5), (2, 3, 5, 4), (1, 2, 6, 7)):
        img, w = torch.randn(2, Ci, H, W, generator=g).double(), torch.randn(Co, Ci, 3, 3, generator=g).double()
        H1, W1 = fm.sub(H), fm.sub(W)
        want = torch.zeros(2, Co, H1, W1, dtype=torch.float64)
        for b in range(2):
            for co in range(Co):
                for t1 in range(H1):
                    for f1 in range(W1):
                        for ci in range(Ci):
                            for kh in range(3):
                                for kw in range(3):
                                    t, f = 2 * t1 - 1 + kh, 2 * f1 - 1 + kw
                                    if 0 <= t < H and 0 <= f < W:
                                        want[b, co, t1, f1] += img[b, ci, t, f] * w[co, ci, kh, kw]
        assert torch.allclose(fm.conv64(img, w), want, rtol=0, atol=1e-13)
        # a dropped tap is that product gone from the masked cells, nowhere else
        kh, kw, mask = fm.drop_of({"tap_dropped_bottom"}, H, W)
        got = fm.conv64(img, w, (kh, kw, mask))
        t = 2 * (H1 - 1) - 1 + kh
        assert t == H - 1
        assert torch.equal(got[:, :, :H1 - 1], fm.conv64(img, w)[:, :, :H1 - 1])


def test_conv1_model_is_the_reference_module_and_the_merged_rule():
    """Conv2d(1, C, 3, 2, 1) + ReLU of the reference on an utterance cut to its own frames, rows past them zero."""
    c = fm.c1("t", "t", "plain", 3, 9, 7, 64, 0, "f32")
    x = torch.randn(3, 9, 7, generator=torch.Generator().manual_seed(2))
    frames = np.array([9, 4, 1])
    m = fm.conv1_model(c, "bf16", x, frames)
    w9c, bias = fm.weights1(64)
    conv = torch.nn.Conv2d(1, 64, 3, 2, 1).double()
    conv.weight.data = w9c.double().t().reshape(64, 1, 3, 3)
    conv.bias.data = bias.double()
    for b, fr in enumerate(frames):
        want = torch.relu(conv(x[b:b + 1, None, :fr].double())).permute(0, 2, 3, 1)[0]
        t1 = want.shape[0]
        assert t1 == fm.sub(fr)
        assert torch.allclose(m["ref"][b, :t1], want, rtol=0, atol=1e-13)
        assert bool((m["ref"][b, t1:] == 0).all()) and bool((m["d"][b, t1:] == 0).all())


def test_conv2_and_linear_models_are_the_reference_modules():
    c = fm.c2("t", "t", "generic", 2, 5, 6, 64, "f32", halo=0)
    v = fm.conv2_values(c)
    m = fm.conv2_model(c, "bf16", {"v": v.double()})
    w2, b2 = fm.weights2(64)
    want = torch.relu(Fn.conv2d(v.double().permute(0, 3, 1, 2), w2.double().permute(0, 3, 1, 2), b2.double(), stride=2, padding=1))
    assert torch.allclose(m["ref"], want.permute(0, 2, 3, 1).reshape(-1, 64), rtol=0, atol=1e-12)
    # the bordered image gives the same rows
    cb = dict(c, halo=1)
    full = torch.zeros(2, 7, 8, 64, dtype=torch.float64)
    full[:, 1:-1, 1:-1] = v.double()
    assert torch.allclose(fm.conv2_model(cb, "bf16", {"v": full})["ref"], m["ref"], rtol=0, atol=1e-12)
    cl = fm.lin("t", "t", "generic", 9, 128, prec="f32", period=4)
    ml = fm.linear_model(cl, "bf16")
    A, _, _ = fm.linear_inputs(cl, "bf16")
    w, b = fm.weights_lin(128)
    want = (A @ w.double().t() + b.double()) * 16.0 + fm.pe_table(cl).double()[torch.arange(9) % 4]
    assert torch.allclose(ml["ref"], want, rtol=0, atol=1e-12)


def test_expand_meta_and_the_layout_maps():
    assert fm.expand_meta([(2, 5), (1, 8), (3, 1)], 6).tolist() == [[5, 2, 0, 2], [5, 2, 0, 2], [8, 2, 2, 3], [1, 1, 3, 6], [1, 1, 3, 6], [1, 1, 3, 6]]
    shape = (2, 3, 4, 64)
    v = (torch.relu(torch.randn(shape, generator=torch.Generator().manual_seed(3))) * 3).double()
    for fmt in fm.IMG_BYTES:
        buf = np.zeros(int(np.prod(shape)) * fm.IMG_BYTES[fmt], np.uint8)
        planes = fm.raw(buf, fmt, shape)
        fm.put(planes, fm.encode(v, fmt, "bf16", 8.0, 1.0))
        assert sum(a.size * a.itemsize for a in planes.values()) == buf.size  # the planes tile the buffer
        val = fm.values(planes, fmt, "bf16", shape, 8.0, 1.0)
        for name, got in fm.views(val, fmt, "bf16").items():
            ref, bound = fm.view_bounds(v, torch.zeros_like(v), fmt, "bf16", 8.0, 1.0, hi=val.get("hi"))[name]
            assert bool(((got - ref).abs() <= bound).all()), (fmt, name)
    # split-bf16 rows: channel c's hi half at byte (c >> 5) * 128 + (c & 31) * 2 of the cell's row, lo 64 bytes further (cn_split_off)
    buf = np.zeros(64 * 4, np.uint8)
    p = fm.raw(buf, "x3", (1, 64))
    p["hi"][0].flat[37] = 0x1234
    p["lo"][0].flat[37] = 0x5678
    off = (37 >> 5) * 128 + (37 & 31) * 2
    assert buf[off:off + 2].view(np.int16)[0] == 0x1234 and buf[off + 64:off + 66].view(np.int16)[0] == 0x5678


def test_mix_emulation_against_the_unsplit_product():
    """MIX: the model of the arithmetic is the three-term product on the planes' bytes.  Its distance from the float64 product of
    the unsplit values (the image's float32 values, the weights' float32 values) against the representational error conv2.hip
    documents: per product, l rounds what half(v) leaves (|.| <= 2^-11 |v|) to four bits and meets q, v at four bits:
    2 (2^-11 (2^-4 + 2^-11) + 2^-15 (1 + 2^-4)) + 2^-22 < 2^-13 of sum |a||w| in the worst case, about 2^-16 per term as an RMS."""
    c = next(c for c in fm.CASES if c["name"].startswith("conv2_mix-B3"))
    m = fm.conv2_model(c, "bf16", fm.conv2_planes(c, "bf16", fm.conv2_image(c, "bf16")))
    v = fm.conv2_values(c).double()
    full = torch.zeros(c["B"], c["T1"] + 2, c["F1"] + 2, c["C"], dtype=torch.float64)
    full[:, 1:-1, 1:-1] = v
    w2, b2 = fm.weights2(c["C"])
    cu = dict(c, form="generic", prec="f32")
    exact = fm.conv2_model(cu, "bf16", {"v": full})
    A = Fn.unfold(full.permute(0, 3, 1, 2).abs(), 3, stride=2)
    S = torch.einsum("bkm,nk->bmn", A.view(c["B"], c["C"], 9, -1).permute(0, 2, 1, 3).reshape(c["B"], 9 * c["C"], -1),
                     w2.reshape(c["C"], -1).abs().double()).reshape(-1, c["C"]) + b2.abs().double()
    live = exact["ref"] > 0
    dist = (m["ref"] - exact["ref"]).abs()[live]
    rel = float(dist.pow(2).mean().sqrt() / exact["ref"][live].pow(2).mean().sqrt())
    print(f"MIX emulation - float64 product of the unsplit values: worst {float((dist / S[live]).max()):.3e} of sum |a||w| (bound 2^-13 = "
          f"{2.0 ** -13:.3e}), rms {rel:.3e} of the rms output")
    assert bool((dist <= 2.0 ** -13 * S[live]).all())
    assert rel < 2.0 ** -13


def test_every_mistake_has_a_predicate_and_the_case_list_covers_what_the_issue_names():
    assert set(APPLIES) == set(fm.MISTAKES)
    names = [c["name"] for c in fm.CASES]
    assert len(set(names)) == len(names)
    k1 = [c for c in fm.CASES if c["kind"] == "conv1"]
    valu = [c for c in k1 if c["form"] not in ("f8m", "m16")]
    assert {c["C"] for c in valu} == {64, 256} and {1, 2, 9, 10} <= {c["T"] for c in valu} and {6, 7, 80, 83} <= {c["F"] for c in valu}
    assert any(c["B"] * fm.sub(c["T"]) > 2048 for c in valu)
    assert {fm.fmt1(c) for c in valu if c["B"] * fm.sub(c["T"]) > 2048} == set(fm.IMG_BYTES)
    assert {f for c in k1 if c["subs"] for _, f in c["subs"]} >= {1, 2, 7, 8, 13}
    assert any(c["halo"] == 2 and c["prev"] and c["subs"] for c in k1)
    mf = [c for c in k1 if c["form"] in ("f8m", "m16")]
    assert {59, 61, 62, 80, 126} <= {c["F"] for c in mf}
    for c in mf:
        if BIG(c):
            P = (fm.sub(c["T"]) + 2) * (fm.sub(c["F"]) + 2)
            nblk = -(-P // 128)
            assert c["B"] * nblk > 1024 and nblk > 1 and 1024 % nblk != 0 and c["subs"]  # block g + 1024 is another utterance's
    k2 = [c for c in fm.CASES if c["kind"] == "conv2"]
    for form in ("dma", "x3", "mix", "f8"):
        Ms = [c["B"] * fm.sub(c["T1"]) * fm.sub(c["F1"]) for c in k2 if c["form"] == form and not c["c1form"]]
        assert min(Ms) < 256 and any(M > 256 and M % 256 for M in Ms), form
        assert {(c["T1"] % 2, c["F1"] % 2) for c in k2 if c["form"] == form} >= {(1, 0), (1, 1), (0, 0)}, form
        assert any(fm.sub(c["F1"]) == 20 and c["B"] > 1 for c in k2 if c["form"] == form), form
        assert {c["halo"] for c in k2 if c["form"] == form and c["c1form"]} == {1, 2}, form
    assert {(c["prec"], c["C"]) for c in k2 if c["form"] == "generic" and not c["halo"]} == {(p, C) for p in ("16", "f32", "x3") for C in (64, 128)} | {("f32", 256)}
    kl = [c for c in fm.CASES if c["kind"] == "linear"]
    assert {c["K"] for c in kl} == {128, 1024, 5120} and {c["M"] for c in kl} == {1, 257}
    assert any(c["lda"] != c["K"] for c in kl) and any(not c["pe"] for c in kl) and all(257 % c["period"] for c in kl)
    assert any(c["form"] == "f8" and c["K"] == 5120 for c in kl)
    # the float64 model stays small: a few thousand rows
    assert max(c["B"] * fm.sub(c["T1"]) * fm.sub(c["F1"]) for c in k2) <= 4096 and max(c["M"] for c in kl) <= 4096


@pytest.mark.parametrize("layout", fm.LIBS)
def test_the_emulation_alone_passes_every_case(layout):
    for c in fm.CASES:
        if layout in c["libs"]:
            fm.run_case(c, layout, fm.emulate)


@pytest.mark.parametrize("mistake", fm.MISTAKES)
def test_mistake_is_caught(mistake):
    cases = [c for c in fm.CASES if APPLIES[mistake](c) and not BIG(c)]
    assert cases, "no case of the GPU test can show this mistake"
    caught, layouts = {}, set()
    for c in cases:
        for layout in c["libs"]:
            layouts.add(layout)
            if layout in caught:
                continue
            old = []
            try:
                fm.run_case(c, layout, lambda call: fm.emulate(call, (mistake,)), oldnorm=old)
            except fm.LaunchError as e:
                was = f"max-norm {max(old):.1e}" if old else "(outside the value tensor)"
                caught[layout] = FOUND[(mistake, layout)] = (e.kind, c["name"], e.ratio, was)
    assert set(caught) == layouts, f"{mistake}: not caught in {layouts - set(caught)}"
    # room above RATIO: a mistake in the values moves the aggregate ratio far past what a correct launch is allowed
    for layout, (kind, name, ratio, _) in caught.items():
        if kind in ("bound", "ratio"):
            assert ratio > 10 * max(fm.RATIO[layout].values()) or ratio != ratio, (mistake, layout, ratio)


def test_old_max_norm_on_a_dropped_conv2_tap():
    """The claim behind the suite, measured: the centre tap of conv2 dropped on the top row of every utterance (256 of an output's
    2304 products gone) against the suite's earlier measure, max |got - ref| / max |ref| over the tensor, and against the
    per-element bound."""
    c = next(c for c in fm.CASES if c["name"].startswith("conv2_dma-B3"))
    pv = fm.conv2_planes(c, "bf16", fm.conv2_image(c, "bf16"))
    m = fm.conv2_model(c, "bf16", pv)
    C, T2, F2 = c["C"], fm.sub(c["T1"]), fm.sub(c["F1"])
    w = fm.r16(fm.weights2(C)[0].double(), "bf16")[:, 1, 1, :]                   # [co][ci] of tap (1, 1)
    contrib = pv["v"][:, 1, 1:1 + 2 * F2:2, :] @ w.t()                            # [B][F2][co]: image row t1 = 0, columns f1 = 2 f2
    got = m["emu"].clone().view(c["B"], T2, F2, C)
    got[:, 0] = torch.where(got[:, 0] > 0, torch.relu(got[:, 0] - contrib), got[:, 0])
    got = got.view(-1, C)
    err = (got - m["ref"]).abs()
    old = float(err.max() / m["ref"].abs().max())
    worst = float((err / (m["d"] + 0.5 * fm.ulp(m["ref"].abs() + m["d"], "bf16")).clamp(min=1e-300)).max())
    print(f"conv2, tap (1, 1) dropped on the top row: old max-norm measure {old:.2e} (thresholds 1.2e-2 bf16, 5e-3 the tightest); "
          f"per-element |err| / bound up to {worst:.1f}")
    assert worst > 4
