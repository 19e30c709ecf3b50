"""LM shallow fusion of the AST beam search (src/models/transformer.py:186-209) and beams / candidate lists up to 32 wide, on the
device: the TransformerLM's incremental step (cn_lm_step), the fused decode (cn_decode_ast with lm_weight > 0), the host-bookkeeping
variant (cn_ast_step_lm) and ArtTask through decode_asr.py.  Fixtures are the reference's own beam_decode with its own
TransformerLM (tools/make_ast_lm_goldens.py; inputs in tests/ast_lm_cases.py)."""
import numpy as np
import pytest
import torch

from ast_lm_cases import CASES, lm_step_prefixes
from conftest import load_golden
from cassnat_asr_public_amd.models import make_conformer, make_transformer
from cassnat_asr_public_amd.models.lm import make_model as make_lm

pytestmark = pytest.mark.gpu


class Vocab:
    word2index = {"blank": 0, "sos": 1, "eos": 2, "unk": 3}


def load(model, state):
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[k]))
    return model


def build(name, prec, host_beam=False):
    args, state, feats, lm_args, lm_state, _ = CASES[name]()
    args.hip_precision, args.hip_host_beam = prec, host_beam
    make = make_conformer if getattr(args, "model_type", "transformer") == "conformer" else make_transformer
    model = load(make(args.input_size, args).cuda(), state)
    lm = None
    if lm_args is not None:
        lm_args.hip_precision = prec
        lm = load(make_lm(lm_args).cuda(), lm_state)
    return args, model, lm, feats


def run(name, prec, host_beam=False):
    args, model, lm, feats = build(name, prec, host_beam)
    src = torch.from_numpy(feats)
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    with torch.no_grad():
        return model.beam_decode(src.cuda(), mask.cuda(), Vocab, args, lm)


def agreement(beams, g):
    exact, total, top1 = 0, 0, 0
    for b, utt in enumerate(beams):
        for j, s in enumerate(utt):
            ok = s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist()
            exact += ok
            total += 1
            top1 += ok and j == 0
    return exact, total, top1


# ------------------------------------------------------------------------------------------------------- the LM step alone
@pytest.mark.parametrize("prec,tol", [("fp32", 1e-5), ("bf16x3", 1e-3)])
def test_lm_step_matches_the_reference_position_by_position(prec, tol):
    """cn_lm_step on every position of token rows that hold blanks (masked keys), the cache written step by step, against the
    reference's lm_model(ys, (ys != 0) & subsequent_mask)[:, -1]; rows without a blank also against cn_lm_score."""
    g = load_golden("ast_lm_step_tiny")
    _, _, _, lm_args, lm_state, _ = CASES["ast_lm_tiny_att"]()
    lm_args.hip_precision = prec
    lm = load(make_lm(lm_args).cuda(), lm_state)
    ys = lm_step_prefixes()
    n, L = ys.shape
    V = lm_args.vocab_size
    eng = lm.step_engine(n)
    eng.lm_step_begin(L, n)
    got = np.zeros((n, L, V), np.float32)
    tok_all = torch.from_numpy(ys).cuda()
    anc = torch.arange(n, dtype=torch.int32).view(n, 1).repeat(1, L).contiguous().cuda()  # slot k wrote every position of row k
    keyok = torch.from_numpy((ys != 0).astype(np.uint8)).cuda()
    out = torch.empty(n, V, dtype=torch.float32, device="cuda")
    for p in range(L):
        eng.lm_step(p, tok_all[:, p].contiguous(), anc, keyok, out)
        got[:, p] = out.cpu().numpy()
    assert np.abs(got - g["lm_logp"]).max() < tol
    rows = [r for r in range(n) if not (ys[r] == 0).any()]
    assert len(rows) >= 2
    tok = torch.from_numpy(ys[rows]).cuda()
    tgt = torch.from_numpy(np.roll(ys[rows], -1, axis=1)).cuda()
    score = lm.score_tokens(tok, tgt, torch.full((len(rows),), L, dtype=torch.int32, device="cuda"), L - 1, max_frames=64).cpu().numpy()
    want = np.take_along_axis(got[rows], np.roll(ys[rows], -1, axis=1)[:, :, None].astype(np.int64), 2)[:, :, 0]
    assert np.abs(score[:, : L - 1] - want[:, : L - 1]).max() < tol


# ------------------------------------------------------------------------------------------------- fused beam search, tiny
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["ast_lm_tiny_att", "ast_lm_tiny_ctc", "ast_lm_tiny_lp"])
def test_ast_lm_tiny_all_beams(name, prec):
    g = load_golden(name)
    beams = run(name, prec)
    for b, utt in enumerate(beams):
        assert len(utt) == g["beam_hyp"].shape[1]
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)
            assert abs(s["score"] - g["beam_score"][b, j]) < max(5e-3, 1e-6 * abs(g["beam_score"][b, j]))


@pytest.mark.parametrize("name", ["ast_lm_tiny_att", "ast_lm_tiny_lp"])
def test_ast_lm_tiny_host_beam(name):
    """The Python-bookkeeping variant over cn_ast_step_lm mirrors the reference literally."""
    g = load_golden(name)
    beams = run(name, "fp32", host_beam=True)
    for b, utt in enumerate(beams):
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)


# ------------------------------------------------------------------------------------- config-4 shapes, beams 10 / 20 wide
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["ast_lm_c4", "ast_wide_c4", "conf_ast_lm_recipe"])
def test_ast_lm_config4(name, prec, capsys):
    """config-4 decoder + lm_small (beam 10), the widening alone (beam 20 / ctc_beam 30, no LM) and run_art.sh stage 3's shape
    (conformer AST, lm.yaml-shaped LM, beam 20 / ctc_beam 30, ctc 0.4, lm 0.6).  The best hypothesis is exact.  Over 20 beams
    neighbours sit 1e-4 .. 1e-3 apart (ast_wide_c4), below the split-bf16 engine's rounding over 30 steps: there the ranked SCORES
    must equal the reference's position by position (a swap of two near-tied beams keeps them), and at most two beams per
    utterance may differ; beam 10 allows two in all."""
    g = load_golden(name)
    beams = run(name, prec)
    exact, total, top1 = agreement(beams, g)
    with capsys.disabled():
        print(f"\n[AST+LM {prec}] {name}: {exact}/{total} beams identical, top-1 identical for {top1}/{len(beams)} utterances")
    assert top1 == len(beams)
    bw = g["beam_hyp"].shape[1]
    assert exact >= total - (2 * len(beams) if bw > 10 else 2)
    for b, utt in enumerate(beams):
        for j, s in enumerate(utt):
            assert abs(s["score"] - g["beam_score"][b, j]) < max(5e-3, 1e-6 * abs(g["beam_score"][b, j])), (b, j)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_ast_lm_c4_half_precision_report(prec, capsys):
    g = load_golden("ast_lm_c4")
    beams = run("ast_lm_c4", prec)
    exact, total, top1 = agreement(beams, g)
    prefix = []
    for b, utt in enumerate(beams):
        ref = g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist()
        got = utt[0]["hyp"]
        k = 0
        while k < min(len(ref), len(got)) and ref[k] == got[k]:
            k += 1
        prefix.append(k)
        assert np.isfinite(utt[0]["score"])
    with capsys.disabled():
        print(f"\n[AST+LM {prec}] beams identical {exact}/{total}, top-1 identical {top1}/{len(beams)}, common prefix of best {prefix}")
    # measured: bf16 7/20 beams, best hypotheses diverging after 2 and 31 tokens; fp16 18/20, [31, 31].  With random weights
    # the V = 5000 distributions are flat and the bf16 LM's log-probabilities are 0.02 off on average (test_gpu_edges), so
    # near-ties flip early; a broken fusion shows as no hypothesis surviving at all
    assert exact >= 3 and max(prefix) >= 15


@pytest.mark.parametrize("name", ["ast_lm_c4", "ast_lm_tiny_att"])
def test_ast_lm_device_beam_equals_host_beam_bf16(name):
    """Same engine, same kernels: the device bookkeeping with the LM term equals the host's bit for bit."""
    dev_b = run(name, "bf16")
    host_b = run(name, "bf16", host_beam=True)
    for u, v in zip(dev_b, host_b):
        assert [s["hyp"] for s in u] == [s["hyp"] for s in v]
        assert [s["score"] for s in u] == [s["score"] for s in v]


def test_lm_weight_without_lm_is_refused():
    args, model, _, feats = build("ast_lm_tiny_ctc", "fp32")
    src = torch.from_numpy(feats)
    with pytest.raises(ValueError, match="lm_model"):
        model.beam_decode(src.cuda(), None, Vocab, args, None)


# ------------------------------------------------------------------------------------------------------ decode_asr --task art
def test_decode_asr_cli_task_art_with_lm(tmp_path):
    """run_art.sh stage 3's options on the tiny fixture: ctc_att, ctc_weight 0.4, --lm_weight 0.6, --lm_config / --rnnlm with
    the checkpoint under "state_dict" (art_task.py:79-84): the result file holds the reference's best beam."""
    import yaml

    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.data import kaldi_io

    g = load_golden("ast_lm_tiny_ctc")
    args, state, feats, lm_args, lm_state, _ = CASES["ast_lm_tiny_ctc"]()
    lengths = [61, 57, 51]
    scp = str(tmp_path / "feats.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "feats.ark"), scp, [(f"spk-utt{b}", feats[b, :n]) for b, n in enumerate(lengths)])
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("".join(f"w{i}\n" for i in range(args.vocab_size - 4)))
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    lm_ckpt = str(tmp_path / "lm.mdl")
    torch.save({"state_dict": {"module." + k: torch.from_numpy(v) for k, v in lm_state.items()}}, lm_ckpt)
    lm_conf = tmp_path / "lm.yaml"
    lm_conf.write_text(yaml.safe_dump({k: getattr(lm_args, k) for k in ("d_model", "n_head", "d_ff", "N", "dropout")}))
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight", "max_decode_ratio",
                                          "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(vocab_file=str(vocab_file), use_gpu=True, n_features=80, model_type="transformer")
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))
    result = str(tmp_path / "token_results.txt")
    rc = decode_asr.main(["--task", "art", "--test_config", str(cfg), "--data_path", scp, "--resume_model", ckpt,
                          "--result_file", result, "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0",
                          "--lm_config", str(lm_conf), "--rnnlm", lm_ckpt, "--lm_weight", "0.6"])
    assert rc == 0
    lines = open(result).read().splitlines()
    assert [ln.split()[0] for ln in lines] == [f"spk-utt{b}" for b in range(3)]
    for b, ln in enumerate(lines):
        best = g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist()
        eos_at = best.index(2) if 2 in best else len(best)
        assert ln.split()[1:] == [f"w{t - 4}" if t > 3 else "unk" for t in best[:eos_at] if t not in (0, 1)], b
