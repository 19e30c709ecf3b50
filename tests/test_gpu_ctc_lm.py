"""CTC prefix beam search with the TransformerLM in the frame loop (src/utils/beam_decode.py:8-93 with lm_model and
args.ctc_lm_weight > 0) on the device: ctc_beam_decode with a TransformerLM against the reference's own ctc_beam_decode with its
own TransformerLM (fixtures: tools/make_ctc_lm_goldens.py; inputs: tests/ctc_lm_cases.py), and CassNATTask through decode_asr.py."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from ctc_lm_cases import CASES, TINY
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
    src = torch.from_numpy(feats).cuda()
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    return args, model, lm, src, mask, torch.from_numpy(sizes).cuda(), extra


def run(name, prec):
    args, model, lm, src, mask, size, extra = build(name, prec)
    with torch.no_grad():
        return ctc_beam_decode(model, src, mask, size, Vocab, args, lm)


def same_score(got, want):
    """tests/test_gpu_nat_lm.py's rule for a hypothesis score against the reference's."""
    return abs(got - want) < max(5e-3, 1e-6 * abs(want))


def agreement(top, g):
    exact = sum(s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist() for b, utt in enumerate(top) for j, s in enumerate(utt))
    top1 = sum(utt[0]["hyp"] == g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist() for b, utt in enumerate(top))
    return exact, sum(len(u) for u in top), top1


def assert_every_entry(top, g):
    assert len(top) == g["beam_hyp"].shape[0]
    for b, utt in enumerate(top):
        assert len(utt) == int(g["beam_n"][b])
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)
            for key, name in (("score_ctc", "beam_score"), ("score_lm", "beam_score_lm"), ("p_blk", "beam_p_blk"), ("p_nblk", "beam_p_nblk")):
                assert isinstance(s[key], float)
                assert same_score(s[key], g[name][b, j]), (b, j, key, s[key], g[name][b, j])
            assert s["ys"].dtype == torch.long and s["ys"][0].tolist() == [1] + s["hyp"]


# ----------------------------------------------------------------------------------------------------------- tiny fixtures
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", TINY)
def test_ctc_lm_tiny_every_beam_entry(name, prec):
    """ctc_only at 0.3 / 5 / 8 / 0.2, beam 1, lp 0 with a small weight, an utterance that skips a frame the others process, the
    search that feeds ctc_att's forced alignment, conformer blocks: every beam entry of every utterance is the reference's
    (neighbouring sort keys are >= 2e-3 apart in every frame, the engines hold 1e-5 on the log-posteriors)."""
    g = load_golden(name)
    top = run(name, prec)
    assert_every_entry(top, g)
    assert any(s["score_lm"] != 0.0 for utt in top for s in utt)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_ctc_att_on_the_fused_search(prec):
    """decode_type ctc_att: the fused search's best hypotheses feed beam_decode's forced alignment; the decoder's result is the
    reference's."""
    g = load_golden("ctc_lm_tiny_ctcatt")
    args, model, lm, src, mask, size, _ = build("ctc_lm_tiny_ctcatt", prec)
    with torch.no_grad():
        top = ctc_beam_decode(model, src, mask, size, Vocab, args, lm)
        out, _ = model.beam_decode(src, mask, size, Vocab, args, None, top)
    for b, seqs in enumerate(out):
        assert seqs[0]["hyp"] == g["hyp"][b, : g["hyp_len"][b]].tolist()
        assert abs(seqs[0]["score"] - g["score"][b]) < 2e-2  # (tests/test_gpu_ctcbeam.py's bound for the same decoder pass)


def test_a_second_call_on_the_same_engines_gives_the_same_result():
    """No state is left in the cache tables: the same batch again, then another fixture's options, then the first again."""
    args, model, lm, src, mask, size, _ = build("ctc_lm_tiny", "fp32")
    with torch.no_grad():
        a = ctc_beam_decode(model, src, mask, size, Vocab, args, lm)
        b = ctc_beam_decode(model, src, mask, size, Vocab, args, lm)
        args.ctc_beam, args.ctc_lp = 3, 0.0
        ctc_beam_decode(model, src[:2], mask[:2], size[:2], Vocab, args, lm)
        args.ctc_beam, args.ctc_lp = 5, 0.2
        c = ctc_beam_decode(model, src, mask, size, Vocab, args, lm)
    key = lambda top: [[(s["hyp"], s["score_ctc"], s["score_lm"], s["p_blk"], s["p_nblk"]) for s in u] for u in top]
    assert key(a) == key(b) == key(c)
    assert_every_entry(c, load_golden("ctc_lm_tiny"))


def test_weight_zero_with_an_lm_is_the_lm_free_search_and_the_lm_matters():
    args, model, lm, src, mask, size, _ = build("ctc_lm_tiny", "fp32")
    args.ctc_lm_weight = 0
    with torch.no_grad():
        a = ctc_beam_decode(model, src, mask, size, Vocab, args, None)
        b = ctc_beam_decode(model, src, mask, size, Vocab, args, lm)
    key = lambda top: [[(s["hyp"], s["score_ctc"], s["score_lm"], s["p_blk"], s["p_nblk"]) for s in u] for u in top]
    assert key(a) == key(b) and all(s["score_lm"] == 0.0 for u in a for s in u)
    g = load_golden("ctc_lm_tiny")
    assert all(u[0]["hyp"] != g["beam_hyp"][i, 0, : g["beam_len"][i, 0]].tolist() for i, u in enumerate(a))


def test_the_device_loop_equals_the_model_on_the_engines_own_log_posteriors():
    """The exact check of the integer / float64 part: tests/ctc_lm_model.py on the engine's own ctc_out, with the device's own LM
    rows (cn_lm_step from position 0 on every prefix), gives the device's beams - hypotheses and order exact, scores to 1e-8."""
    from ctc_lm_model import fused_search
    from oracle import cassnat_oracle as orc

    args, model, lm, src, mask, size, _ = build("ctc_lm_tiny_skip", "fp32")
    args.hip_capture = True
    with torch.no_grad():
        top = ctc_beam_decode(model, src, mask, size, Vocab, args, lm)
    ctc_dev = model._engine.fetch("ctc_out")
    n_rows = src.shape[0] * args.ctc_beam  # (as many rows as the loop's LM step ran on)
    eng = lm.step_engine(n_rows)
    eng.lm_step_begin(ctc_dev.shape[1] + 2, n_rows)

    def lm_rows(ys, m):
        n, L = n_rows, ys.shape[1]
        anc = torch.arange(n, dtype=torch.int32, device="cuda")[:, None].repeat(1, L).contiguous()
        keyok = torch.ones(n, L, dtype=torch.uint8, device="cuda")
        logp = torch.empty(n, ctc_dev.shape[2], device="cuda")
        for pos in range(L):
            eng.lm_step(pos, torch.full((n,), int(ys[0, pos]), dtype=torch.int32, device="cuda"), anc, keyok, logp)
        torch.cuda.synchronize()
        return logp[0].cpu().numpy()

    want = fused_search(ctc_dev, orc.src_size_frames(size.cpu().numpy(), ctc_dev.shape[1]), args.ctc_beam, args.ctc_pruning, args.ctc_lp,
                        args.ctc_lm_weight, lm_rows)
    for b, utt in enumerate(top):
        assert [s["hyp"] for s in utt] == [s["hyp"] for s in want[b]]
        for key in ("score_ctc", "score_lm", "p_blk", "p_nblk"):
            np.testing.assert_allclose([s[key] for s in utt], [s[key] for s in want[b]], rtol=0, atol=1e-8, err_msg=key)


# ------------------------------------------------------------------------------------------------------------ config-2 shape
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_ctc_lm_config2_best_hypothesis(prec, capsys):
    """config 2 + lm_small, 300 / 231 frames, ctc_beam 5, ctc_pruning 8: the reference's smallest neighbouring key gap is 1.8e-4
    (four below 1e-3), so the best hypothesis of both utterances is required and the rest is reported."""
    g = load_golden("ctc_lm_config2")
    top = run("ctc_lm_config2", prec)
    exact, total, top1 = agreement(top, g)
    with capsys.disabled():
        print(f"\n[CTC+LM {prec}] ctc_lm_config2: {exact}/{total} beam entries identical, best identical for {top1}/{len(top)} utterances")
    assert top1 == len(top)
    for b, utt in enumerate(top):
        assert same_score(utt[0]["score_ctc"], g["beam_score"][b, 0]) and same_score(utt[0]["score_lm"], g["beam_score_lm"][b, 0])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_ctc_lm_config2_half_precision_report(prec, capsys):
    g = load_golden("ctc_lm_config2")
    top = run("ctc_lm_config2", prec)
    exact, total, top1 = agreement(top, g)
    with capsys.disabled():
        print(f"\n[CTC+LM {prec}] ctc_lm_config2: {exact}/{total} beam entries identical, best identical for {top1}/{len(top)} utterances")
    assert all(np.isfinite(s["score_ctc"]) and np.isfinite(s["score_lm"]) for utt in top for s in utt)


def test_a_too_small_lm_handle_is_refused_with_the_limit_named():
    from cassnat_asr_public_amd import hip

    args, model, lm, src, mask, size, _ = build("ctc_lm_tiny", "fp32")
    eng = model.engine(src.shape[0], src.shape[1])
    small = lm.new_engine(1, lm.engine(1, 4))  # one slot
    opts = hip.Engine.make_opts(args)
    with pytest.raises(hip.HipError, match="15 beam slots"):
        eng.ctc_beam_lm(small, src.float().contiguous(), size.float().contiguous(), opts, 5, 8, 0.2, 0.3)
    small.close()


# -------------------------------------------------------------------------------------------------- decode_asr --task cassnat
@pytest.mark.parametrize("name", ["ctc_lm_tiny", "ctc_lm_tiny_ctcatt"])
def test_decode_asr_cli_task_cassnat_with_ctc_lm_weight(tmp_path, name):
    """`decode_type: ctc_only / ctc_att` with `ctc_lm_weight > 0` in the YAML and --lm_config / --rnnlm on the command line: the
    result file holds the reference's text."""
    import yaml

    from oracle import cassnat_oracle as orc
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.bin import decode_asr

    g = load_golden(name)
    args, state, feats, sizes, lm_args, lm_state, extra = CASES[name]()
    conf = {k: getattr(args, k) for k in ("decode_type", "sample_num", "ctc_beam", "ctc_pruning", "ctc_lp", "ctc_lm_weight")}
    scp, ckpt, cfg = _write_case(tmp_path, args, state, feats, [61, 50, 37], extra_conf=conf)
    lm_ckpt = str(tmp_path / "lm.mdl")
    torch.save({"model_state": {"module." + k: torch.from_numpy(v) for k, v in lm_state.items()}}, lm_ckpt)
    lm_conf = tmp_path / "lm.yaml"
    lm_conf.write_text(yaml.safe_dump({k: getattr(lm_args, k) for k in ("d_model", "n_head", "d_ff", "N", "dropout")}))
    result = str(tmp_path / "token_results.txt")
    rc = decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                          "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0", "--lm_config", str(lm_conf),
                          "--rnnlm", lm_ckpt, "--rank_model", "lm"])
    assert rc == 0
    index2word = {i + 4: f"w{i}" for i in range(args.vocab_size - 4)}
    index2word[3] = "unk"
    if extra.get("ctc_att"):
        best = [g["hyp"][b, : g["hyp_len"][b]].tolist() for b in range(3)]
    else:
        best = [g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist() for b in range(3)]
    expect = [f"spk-utt{b:02d} " + " ".join(orc.hyp_to_text(h, index2word)) for b, h in enumerate(best)]
    assert open(result).read().splitlines() == expect
