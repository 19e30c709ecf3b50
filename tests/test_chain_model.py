"""The checks of chain_model.py would catch what a row-chain kernel can get wrong - shown on the CPU, on the case list the GPU test
(test_gpu_chain.py) runs.  A launch is stood in for by the model's EMULATION (every intermediate rounding applied, float64
accumulation) writing the launch's buffers:

* the correct emulation passes every case in both layouts: the bounds hold for the roundings the kernel applies, the aggregate
  ratio is 1 by construction, nothing outside the launch's own elements is written (the "reference alone" condition);
* the emulation with one deliberate mistake fails at least one case - the per-element bound, the aggregate check or an untouched
  sentinel.  The table (-s) names the check and the layout that catches each mistake.

The two LayerNorm mistakes of 0.2 % (the biased std: sqrt(255 / 256)) must be caught in the fp16 layout; in the bf16 layout the
operand's own roundoff (2^-9 = 0.2 %) is as large as they are, they stay inside every bound and move the RMS by a factor that is
reported here, not required: that is why the kernel is tested in both libraries.

The two row mistakes, as this test reads them: with the row count on the device (rows < M) the last live row of a partial 32-row
block is computed from row M - 1 of the inputs (clamp_to_capacity: the clamp took the host's count), and the reverse, its results
are stored at row M - 1 (store_at_capacity)."""
import pytest
import torch

import chain_model as cm

FOUND = {}

# the cases a mistake can show on
APPLIES = {
    "ln1_biased_std": lambda c: c["dff"] > 0,
    "lnn_biased_std": lambda c: c["has_next"],
    "ln1_eps_in_var": lambda c: c["dff"] > 0 and c["adv"],
    "lnn_eps_in_var": lambda c: c["has_next"] and c["adv"] and not c["dff"],
    "no_b1": lambda c: c["dff"] > 0,
    "no_b2": lambda c: c["dff"] > 0,
    "no_bo": lambda c: c["ctx"],
    "no_bt": lambda c: c["tail"] > 0,
    "no_residual_attn": lambda c: c["ctx"],
    "no_residual_ffn": lambda c: c["dff"] > 0,
    "act_swapped": lambda c: c["dff"] > 0,
    "lnn_uses_ln1_vectors": lambda c: c["has_next"],
    "ldctx_ignored": lambda c: c["ctx"] == "rm" and c["ldctx"] != cm.D,
    "clamp_to_capacity": lambda c: c["rows"] is not None and c["rows"] % 32,
    "store_at_capacity": lambda c: c["rows"] is not None and c["rows"] % 32 and not (c["out_blk"] or c["ln_blk"]),
    "xin_blk_chunks": lambda c: c["xin_blk"],
    "xout_blk_chunks": lambda c: c["xout_blk"] and c["store_x"],
    "ctx_blk_chunks": lambda c: c["ctx"] == "blk",
    "out_blk_chunks": lambda c: c["tail"] > 0 and c["out_blk"],
    "ln_blk_chunks": lambda c: c["ln_blk"],
    "tail_tile_shifted": lambda c: c["tail"] > 0,
}
SMALL = ("ln1_biased_std", "lnn_biased_std")  # 0.2 %: below the bf16 operand's roundoff


def run(c, layout, mistakes=()):
    before = cm.buffers(c, layout)
    after = {k: (None if v is None else v.clone()) for k, v in before.items()}
    cm.emulate_launch(c, layout, after, mistakes)
    cm.check_launch(c, layout, before, after)


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nmistake: what catches it first per layout (check, case, rms ratio of an aggregate failure)")
    for (name, layout), (kind, case, ratio) in sorted(FOUND.items()):
        print(f"  {name:22s} {layout:5s} {kind:10s} {case:40s} {'' if ratio is None else f'{ratio:.1f}'}")


def test_every_mistake_has_a_predicate_and_the_index_maps_are_the_permutations():
    assert set(APPLIES) == set(cm.MISTAKES)
    for M in (1, 33, 64):
        x = torch.randn(M, cm.D)
        blk = cm.to_blocked_x(x).reshape(-1)
        assert torch.equal(blk[cm.xblk_index(M)], x)
        assert torch.equal(cm.from_blocked_x(blk.view(-1, 32, 64, 4), M), x)
        for N in (256, 768):
            t = torch.randn(cm.rows32(M) * N)
            assert torch.equal(t[cm.blk16_index(M, N)], cm.from_blocked16(t, M, N))
        # the blocked LNn(x) is the blocked ctx with the channels in the accumulator's order
        c = torch.arange(cm.D)
        acc = 32 * (c // 32) + 16 * (c % 32 // 16) + 8 * (c % 8 // 4) + 4 * (c % 16 // 8) + c % 4  # position c holds channel acc[c]
        assert sorted(acc.tolist()) == list(range(cm.D))
        assert torch.equal(cm.lnblk_index(M)[:, acc], cm.oblk_index(M))
    names = [c["name"] for c in cm.CASES]
    assert len(set(names)) == len(names)


def test_case_list_covers_what_the_issue_names():
    by = {}
    for c in cm.CASES:
        by.setdefault(c["name"].split("-M")[0], []).append(c)
    for form, cs in by.items():
        live = {c["M"] if c["rows"] is None else c["rows"] for c in cs}
        assert {1, 33, 129} <= live, form
        assert max(c["M"] for c in cs) <= 257 + 131 and max(live) <= 257, form
        assert sum(c["adv"] for c in cs) == 1, form
        if form.startswith("enc_layer_") or form.startswith("enc_last"):
            assert set(cm.M_ALL) <= live, form
        if form.startswith("dec_"):
            assert all(c["rows"] is not None and c["M"] > cm.rows32(c["rows"]) + 96 for c in cs), form  # an idle workgroup
    assert any(c["ldctx"] != cm.D for c in cm.CASES) and any(c["swish"] and c["ctx"] for c in cm.CASES)
    assert {c["tail"] for c in cm.CASES if c["swish"]} == {0, 256, 512, 768}
    assert any(not c["ctx"] and not c["dff"] and not c["tail"] for c in cm.CASES)                    # NG = 0
    assert any(c["ctx"] and not c["dff"] and not c["has_next"] for c in cm.CASES)                    # NG = 1
    assert any(c["dff"] == 128 for c in cm.CASES) and any(c["dff"] == 2048 and c["tail"] == 1536 and c["ctx"] for c in cm.CASES)


@pytest.mark.parametrize("layout", cm.LIBS)
def test_the_emulation_alone_passes_every_case(layout):
    for c in cm.CASES:
        run(c, layout)


@pytest.mark.parametrize("mistake", cm.MISTAKES)
def test_mistake_is_caught(mistake):
    cases = [c for c in cm.CASES if APPLIES[mistake](c)]
    assert cases, "no case of the GPU test can show this mistake"
    caught = {}
    for layout in cm.LIBS:
        for c in cases:
            try:
                run(c, layout, (mistake,))
            except cm.LaunchError as e:
                caught[layout] = FOUND[(mistake, layout)] = (e.kind, c["name"], e.ratio)
                break
    assert "fp16" in caught, f"{mistake}: no case catches it in the fp16 layout"
    if mistake not in SMALL:
        assert "bf16" in caught, f"{mistake}: no case catches it in the bf16 layout"


@pytest.mark.parametrize("layout", cm.LIBS)
def test_room_between_the_emulation_and_the_smallest_mistake(layout):
    """RATIO sits between what a correct launch measures (chain_model.RATIO's comment) and the smallest aggregate ratio of a
    mistake the bounds do not see: where a 0.2 % LayerNorm mistake is inside every bound, it must move the RMS well past RATIO in
    the fp16 layout on every case it applies to (twice RATIO at the least; the bf16 figures are printed only)."""
    worst = {}
    for mistake in SMALL:
        ratios = []
        for c in [c for c in cm.CASES if APPLIES[mistake](c)][:12]:
            before = cm.buffers(c, layout)
            after = {k: (None if v is None else v.clone()) for k, v in before.items()}
            cm.emulate_launch(c, layout, after, (mistake,))
            seen, kind = {}, None
            try:
                cm.check_launch(c, layout, before, after, seen)
            except cm.LaunchError as e:
                kind = e.kind
            ratios.append(float("inf") if kind in ("bound", "untouched") else max(v[1] for v in seen.values()))
        worst[mistake] = min(ratios)
        print(f"{layout} {mistake}: smallest rms ratio over {len(ratios)} cases {min(ratios):.2f}, largest {max(ratios):.2f}")
    if layout == "fp16":
        assert min(worst.values()) > 2 * cm.RATIO[layout], worst
