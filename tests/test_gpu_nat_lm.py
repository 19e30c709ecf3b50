"""CASS-NAT decoding with LM shallow fusion (src/models/cassnat.py:574-637, args.lm_weight > 0) on the device: CassNAT.beam_decode
with a TransformerLM as lm_model against the reference's own beam_decode with its own TransformerLM (fixtures:
tools/make_nat_lm_goldens.py; inputs: tests/nat_lm_cases.py), and CassNATTask through decode_asr.py."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from nat_lm_cases import CASES, TINY
from cassnat_asr_public_amd.models import make_cassnat_model
from cassnat_asr_public_amd.models.lm import make_model as make_lm
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode

pytestmark = pytest.mark.gpu


class Vocab:
    word2index = {"blank": 0, "sos": 1, "eos": 2, "unk": 3}


def load(model, state):
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[k]))
    return model


def build(name, prec):
    args, state, feats, sizes, lm_args, lm_state, extra = CASES[name]()
    args.hip_precision = lm_args.hip_precision = prec
    model = load(make_cassnat_model(args.input_size, args).cuda(), state)
    lm = load(make_lm(lm_args).cuda(), lm_state)
    return args, model, lm, feats, sizes, extra


def run(name, prec):
    args, model, lm, feats, sizes, extra = build(name, prec)
    if "select_seed" in extra:
        args.esa_select = load_golden(name)["select"]
    src = torch.from_numpy(feats).cuda()
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    size = torch.from_numpy(sizes).cuda()
    with torch.no_grad():
        top = ctc_beam_decode(model, src, mask, size, Vocab, args, None) if extra.get("ctc_att") else None
        out, _ = model.beam_decode(src, mask, size, Vocab, args, lm, top)
    return out


def same_score(got, want):
    """tests/test_gpu_ast_lm.py's rule for a hypothesis score against the reference's."""
    return abs(got - want) < max(5e-3, 1e-6 * abs(want))


def agreement(beams, g):
    exact, total, top1 = 0, 0, 0
    for b, utt in enumerate(beams):
        for j, s in enumerate(utt):
            ok = s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist()
            exact += ok
            total += 1
            top1 += ok and j == 0
    return exact, total, top1


# ----------------------------------------------------------------------------------------------------------- tiny fixtures
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", TINY)
def test_nat_lm_tiny_every_beam(name, prec):
    """att_only with and without the trigger mask, beam 1, ESA + rank_model lm, ctc_att, conformer blocks: every beam of every
    utterance is the reference's (the sort keys of neighbouring beams are >= 2.6e-2 apart, the engines hold 1e-5), 'ys' has grown
    with the hypothesis as the reference grows it when the LM is on."""
    g = load_golden(name)
    beams = run(name, prec)
    assert len(beams) == g["beam_hyp"].shape[0]
    for b, utt in enumerate(beams):
        assert len(utt) == g["beam_hyp"].shape[1]
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)
            assert same_score(s["score"], g["beam_score"][b, j]), (b, j, s["score"], g["beam_score"][b, j])
            assert isinstance(s["score"], float) and s["ys"].dtype == torch.long
            assert tuple(s["ys"].shape) == (1, len(s["hyp"])) and s["ys"][0].tolist() == s["hyp"]


# ------------------------------------------------------------------------------------------------------------ config-2 shape
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_nat_lm_config2(prec, capsys):
    """config 2 + lm_small, beam 5, hypotheses of 53 and 42 tokens.  Neighbouring final beams sit 1.6e-3 and 3.5e-4 apart, near
    the engines' rounding over 50 steps, so the rule is test_ast_lm_config4's: the best hypothesis identical per utterance, the
    ranked SCORES equal to the reference's position by position (a swap of two near-tied beams keeps them), at most two beams
    differing in all."""
    g = load_golden("nat_lm_config2")
    beams = run("nat_lm_config2", prec)
    exact, total, top1 = agreement(beams, g)
    with capsys.disabled():
        print(f"\n[NAT+LM {prec}] nat_lm_config2: {exact}/{total} beams identical, top-1 identical for {top1}/{len(beams)} utterances")
    assert top1 == len(beams)
    assert exact >= total - 2
    for b, utt in enumerate(beams):
        assert [len(s["hyp"]) for s in utt] == g["beam_len"][b].tolist()
        for j, s in enumerate(utt):
            assert same_score(s["score"], g["beam_score"][b, j]), (b, j)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_nat_lm_config2_half_precision_report(prec, capsys):
    g = load_golden("nat_lm_config2")
    beams = run("nat_lm_config2", prec)
    exact, total, top1 = agreement(beams, g)
    prefix = []
    for b, utt in enumerate(beams):
        ref = g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist()
        got = utt[0]["hyp"]
        k = 0
        while k < min(len(ref), len(got)) and ref[k] == got[k]:
            k += 1
        prefix.append(k)
        assert all(np.isfinite(s["score"]) for s in utt)
    with capsys.disabled():
        print(f"\n[NAT+LM {prec}] beams identical {exact}/{total}, top-1 identical {top1}/{len(beams)}, common prefix of best {prefix}")
    # measured: bf16 3/10 beams, no best hypothesis identical, best hypotheses diverging after 2 and 26 tokens; fp16 5/10 beams, one
    # best hypothesis identical, common prefixes [53, 38] of 53 and 42 tokens.  With random weights the V = 5000 distributions are
    # flat and the bf16 engines' log-probabilities are 0.02 off on average (test_gpu_edges), so near-ties flip early and the
    # alignment itself may differ; a broken fusion shows as no hypothesis and no long prefix surviving at all.  Floor: half of
    # what bf16 showed
    assert exact >= 1 and max(prefix) >= 13


def test_lm_weight_zero_is_untouched_by_the_lm():
    """lm_weight 0 keeps the host beam over the fetched top-k tables, with or without an LM object at hand."""
    args, model, lm, feats, sizes, _ = build("nat_lm_tiny", "fp32")
    args.lm_weight = 0
    src = torch.from_numpy(feats).cuda()
    size = torch.from_numpy(sizes).cuda()
    with torch.no_grad():
        a, _ = model.beam_decode(src, None, size, Vocab, args, None)
        b, _ = model.beam_decode(src, None, size, Vocab, args, lm)
    assert [[(s["hyp"], s["score"]) for s in u] for u in a] == [[(s["hyp"], s["score"]) for s in u] for u in b]
    g = load_golden("nat_lm_tiny")
    assert all(u[0]["hyp"] != g["beam_hyp"][i, 0, : g["beam_len"][i, 0]].tolist() for i, u in enumerate(a))  # the LM matters


def test_lm_weight_without_lm_is_refused():
    args, model, _, feats, sizes, _ = build("nat_lm_tiny", "fp32")
    src = torch.from_numpy(feats).cuda()
    with pytest.raises(ValueError, match="lm_model"):
        model.beam_decode(src, None, torch.from_numpy(sizes).cuda(), Vocab, args, None)


def test_finish_needs_the_rows_of_the_pass():
    """cn_nat_lm_finish after a greedy pass that kept the arg-max alone is an error, not a read of stale rows."""
    from cassnat_asr_public_amd import hip

    args, model, lm, feats, sizes, _ = build("nat_lm_tiny_bw1", "bf16")
    args.lm_weight = 0
    src = torch.from_numpy(feats).cuda()
    with torch.no_grad():
        model.beam_decode(src, None, torch.from_numpy(sizes).cuda(), Vocab, args, None)
    args.lm_weight = 0.3
    opts = hip.Engine.make_opts(args)
    with pytest.raises(hip.HipError, match="kept no log-probability rows"):
        model._lm_finish(model._engine, opts, args, lm, 3, 5, False)


# -------------------------------------------------------------------------------------------------- decode_asr --task cassnat
@pytest.mark.parametrize("name", ["nat_lm_tiny", "nat_lm_tiny_ctcatt"])
def test_decode_asr_cli_task_cassnat_with_lm(tmp_path, name):
    """The recipe's flags (run_hubert.sh: --lm_weight, --lm_config, --rnnlm, --rank_model) on the tiny fixtures - att_only, and
    `decode_type: ctc_att` (the task's own ctc_beam_decode call, then beam_decode with the LM) -, the LM checkpoint under
    "model_state" with the `module.` prefix: the result file holds the reference's best beam per utterance."""
    import yaml

    from oracle import cassnat_oracle as orc
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.bin import decode_asr

    g = load_golden(name)
    args, state, feats, sizes, lm_args, lm_state, extra = CASES[name]()
    conf = {k: getattr(args, k) for k in ("decode_type", "sample_num", "ctc_beam", "ctc_pruning", "ctc_lp", "ctc_lm_weight")} if extra.get("ctc_att") else None
    scp, ckpt, cfg = _write_case(tmp_path, args, state, feats, [61, 50, 37], extra_conf=conf)
    lm_ckpt = str(tmp_path / "lm.mdl")
    torch.save({"model_state": {"module." + k: torch.from_numpy(v) for k, v in lm_state.items()}}, lm_ckpt)
    lm_conf = tmp_path / "lm.yaml"
    lm_conf.write_text(yaml.safe_dump({k: getattr(lm_args, k) for k in ("d_model", "n_head", "d_ff", "N", "dropout")}))
    result = str(tmp_path / "token_results.txt")
    rc = decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                          "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0", "--lm_weight", "0.6",
                          "--lm_config", str(lm_conf), "--rnnlm", lm_ckpt, "--rank_model", "lm"])
    assert rc == 0
    index2word = {i + 4: f"w{i}" for i in range(args.vocab_size - 4)}
    index2word[3] = "unk"
    best = [g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist() for b in range(3)]
    expect = [f"spk-utt{b:02d} " + " ".join(orc.hyp_to_text(h, index2word)) for b, h in enumerate(best)]
    assert open(result).read().splitlines() == expect
