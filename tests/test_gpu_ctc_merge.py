"""The merging CTC prefix beam search end to end on the tiny models: ``Engine.ctc_beam_merged`` (through ctc_beam_decode) against
tests/ctc_merge_model.py and cn_ctc_merged_beam_host run on the engine's own captured log-posteriors and their pruned lists (fp32 and
bf16x3, NAT and AST handles, without fusion, with a phrase list and with an n-gram model), a fixture whose unmerged and merged best
hypotheses differ, and decode_asr --hip_ctc_merge 1 for CassNATTask (ctc_only, ctc_att) and ArtTask (ctc_only), alone, with --hip_bias
and with --rank_model n-gram; --hip_ctc_merge 0 and no flag give the same bytes."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_merge_cases as cases
import ctc_merge_model as model
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.bias import BiasList
from cassnat_asr_public_amd.models.ngram import NgramLM, _ptr
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode
from ctc_ngram_model import WordModel, dyadic_arpa
from test_gpu_ctc_bias import assert_same, ast, lines_of, nat, phrases_of, run_cli, write_list
from test_gpu_ctc_ngram import PIECES40, VOCAB, WEIGHT
from test_gpu_ngram import WORDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    text = dyadic_arpa(WORDS, 3, seed=3)
    path = tmp_path_factory.mktemp("ctc_merge") / "model.arpa"
    path.write_text(text, encoding="utf-8")
    return str(path), text


def search(m, args, batch, vocab, merge, bias=None, lm=None):
    """ctc_beam_decode, and the log-posteriors, pruned lists and frame counts it ran on."""
    with torch.no_grad():
        top = ctc_beam_decode(m, *batch, vocab, args, lm, bias=bias, merge=merge)
    ctc = np.asarray(m.engine(*batch[0].shape[:2]).fetch("ctc_out"), np.float32)
    pruned = torch.topk(torch.from_numpy(ctc), args.ctc_pruning, dim=-1)[1].numpy().astype(np.int32)
    return top, SimpleNamespace(logp=np.ascontiguousarray(ctc), top=np.ascontiguousarray(pruned), ratio=batch[2].cpu().numpy().astype(np.float32),
                                W=int(args.ctc_beam), P=int(args.ctc_pruning), lp=float(args.ctc_lp))


def model_of(case, scorer, blank=0, merge=True):
    return model.search(case.logp, case.top, cases.src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, scorer, blank=blank, merge=merge)


def close(top, want, tol=1e-8):
    """assert_same with score_lm to the tolerance (an ARPA model that is not dyadic in lm_scale)."""
    assert len(top) == len(want)
    for b, utt in enumerate(top):
        assert [s["hyp"] for s in utt] == [s["hyp"] for s in want[b]], b
        for key in ("score_ctc", "score_lm", "p_blk", "p_nblk"):
            np.testing.assert_allclose([s[key] for s in utt], [s[key] for s in want[b]], rtol=0, atol=tol, err_msg=key)


@pytest.mark.parametrize("which", ["nat", "ast"])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_the_engine_equals_the_model_on_its_own_log_posteriors(prec, which, arpa):
    m, args, batch = nat(prec) if which == "nat" else ast(prec)
    free, _ = search(m, args, batch, VOCAB, 0)
    top, case = search(m, args, batch, VOCAB, 1)
    assert_same(top, model_of(case, None, args.padding_idx))
    for utt in top:
        assert len({tuple(s["hyp"]) for s in utt}) == len(utt)
        for s in utt:
            assert s["ys"].dtype == torch.long and s["ys"][0].tolist() == [1] + s["hyp"] and s["score_lm"] == 0.0
    if which == "nat":  # (the unmerged beams of this model do hold duplicates: merging had something to do)
        assert any(len({tuple(s["hyp"]) for s in u}) < len(u) for u in free)
    # with a phrase list
    phrases = phrases_of(free)
    biased, case = search(m, args, batch, VOCAB, 1, bias=BiasList.from_phrases(phrases))
    assert_same(biased, model_of(case, model.BiasScorer(phrases), args.padding_idx))
    assert any(s["score_lm"] != 0.0 for u in biased for s in u)
    # with an n-gram model
    path, text = arpa
    args.ctc_lm_weight, args.rank_model = WEIGHT, "n-gram"
    fused, case = search(m, args, batch, VOCAB, 1, lm=NgramLM.load(path, VOCAB))
    close(fused, model_of(case, model.NgramScorer(WordModel(text), VOCAB, WEIGHT * math.log(10.0)), args.padding_idx))
    assert all(s["score_lm"] < 0.0 for u in fused for s in u)


def test_the_flag_off_is_the_unmerged_search():
    m, args, batch = nat("fp32")
    free, _ = search(m, args, batch, VOCAB, None)
    args.hip_ctc_merge = 0
    off, _ = search(m, args, batch, VOCAB, None)
    key = lambda top: [[(s["hyp"], s["score_ctc"], s["score_lm"], s["p_blk"], s["p_nblk"]) for s in u] for u in top]
    assert key(off) == key(free)
    args.hip_ctc_merge = 1  # (the way decode_asr hands the flag over)
    on, case = search(m, args, batch, VOCAB, None)
    assert_same(on, model_of(case, None, args.padding_idx))
    assert key(on) != key(free)


def test_the_merged_best_is_the_sequence_with_the_larger_probability():
    """Three frames in which label 1 has 0.3 and blank 0.65: the paths that spell "1" come in bundles that are each weaker than the
    all-blank path, so the unmerged search ends with the empty hypothesis on top; summed they outweigh it (0.52 against 0.28)."""
    p = np.array([[[0.65, 0.3, 0.05], [0.66, 0.3, 0.04], [0.65, 0.29, 0.06]]])
    logp = np.log(p).astype(np.float32)
    top = np.tile(np.array([1, 2], np.int32), (1, 3, 1))
    want = model.brute_force(logp[0].astype(np.float64))
    merged_model = model.search(logp, top, [3], 3, 0.0)[0]
    plain_model = model.search(logp, top, [3], 3, 0.0, merge=False)[0]
    assert plain_model[0]["hyp"] == [] and merged_model[0]["hyp"] == [1] and want[(1,)] > want[()]
    assert max(want, key=want.get) == (1,)
    d = SimpleNamespace(logp=torch.from_numpy(logp).cuda(), top=torch.from_numpy(top).cuda(), ratio=torch.ones(1).cuda())
    out = {}
    for name in ("merged", "plain"):
        hyp = torch.zeros(1, 3, 4, dtype=torch.int32, device="cuda")
        hlen, nb = torch.zeros(1, 3, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        sc, slm, pb, pnb = (torch.zeros(1, 3, dtype=torch.float64, device="cuda") for _ in range(4))
        if name == "merged":
            hip.check(hip.lib().cn_op_ctc_merged_beam(None, 0.0, None, _ptr(d.logp), _ptr(d.top), _ptr(d.ratio), 1, 3, 3, 3, 2, 0.0, 0, _ptr(hyp), 4,
                                                      _ptr(hlen), _ptr(sc), _ptr(slm), _ptr(pb), _ptr(pnb), _ptr(nb), hip.current_stream()))
        else:
            hip.check(hip.lib().cn_op_ctc_prefix_beam(_ptr(d.logp), _ptr(d.ratio), 1, 3, 3, 3, 2, 0.0, 0, _ptr(hyp), 4, _ptr(hlen), _ptr(sc),
                                                      _ptr(pb), _ptr(pnb), _ptr(nb), hip.current_stream()))
        torch.cuda.synchronize()
        out[name] = (hyp[0, 0, :int(hlen[0, 0])].tolist(), float(sc[0, 0]))
    assert out["plain"][0] == [] and out["merged"][0] == [1]
    assert abs(out["merged"][1] - want[(1,)]) <= 1e-6 and out["merged"][1] > out["plain"][1]  # (float32 log-posteriors)


# ---- decode_asr ----------------------------------------------------------------------------------------------------------------------
def cassnat_cli(tmp_path, decode_type, conf_more=None):
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.data.vocab import Vocab

    m, args, batch = nat("fp32", decode_type)
    vocab_file = tmp_path / "pieces.txt"
    vocab_file.write_text("".join(p + "\n" for p in PIECES40[4:]), encoding="utf-8")
    vocab = Vocab(str(vocab_file), rank=1)
    conf = dict(dict(decode_type=decode_type, sample_num=1, vocab_file=str(vocab_file), ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0),
                **(conf_more or {}))
    scp, ckpt, cfg = _write_case(tmp_path, args, dict((k, v.detach().cpu().numpy()) for k, v in m.named_parameters()), batch[0].cpu().numpy(),
                                 [61, 50, 37], extra_conf=conf)
    cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "3", "--hip_precision", "fp32",
           "--load_data_workers", "0"]
    return m, args, batch, vocab, cli


@pytest.mark.parametrize("decode_type", ["ctc_only", "ctc_att"])
def test_decode_asr_cassnat_merged(tmp_path, decode_type):
    m, args, batch, vocab, cli = cassnat_cli(tmp_path, decode_type)
    free, _ = search(m, args, batch, vocab, 0)
    top, case = search(m, args, batch, vocab, 1)
    # the model's hypotheses on the engine's log-posteriors; with ctc_att the decoder is aligned to the best of them
    want = model_of(case, None, args.padding_idx)
    recog = [[{"hyp": list(s["hyp"]), "ys": torch.tensor([[1] + s["hyp"]], dtype=torch.long)} for s in u] for u in want]
    plain = free
    if decode_type == "ctc_att":
        with torch.no_grad():
            recog, _ = m.beam_decode(*batch, vocab, args, None, recog)
            plain, _ = m.beam_decode(*batch, vocab, args, None, free)
    got = run_cli(tmp_path, cli, "merged", ["--hip_ctc_merge", "1"])
    assert got.decode("utf-8").splitlines() == lines_of(recog, vocab, args)
    # the flag at 0 and no flag: what the unmerged search gives, the same bytes
    first = run_cli(tmp_path, cli, "plain")
    assert first.decode("utf-8").splitlines() == lines_of(plain, vocab, args) and run_cli(tmp_path, cli, "off", ["--hip_ctc_merge", "0"]) == first


def test_decode_asr_cassnat_merged_with_a_list_and_with_an_arpa_file(tmp_path, arpa):
    path, text = arpa
    m, args, batch, vocab, cli = cassnat_cli(tmp_path, "ctc_only")
    free, _ = search(m, args, batch, vocab, 0)
    phrases = phrases_of(free, low=4)
    _, case = search(m, args, batch, vocab, 1)
    want = model_of(case, model.BiasScorer(phrases), args.padding_idx)
    got = run_cli(tmp_path, cli, "bias", ["--hip_ctc_merge", "1", "--hip_bias", write_list(tmp_path, phrases, vocab)])
    assert got.decode("utf-8").splitlines() == lines_of(want, vocab, args)
    sub = tmp_path / "ngram"
    sub.mkdir()
    m, args, batch, vocab, cli = cassnat_cli(sub, "ctc_only", dict(ctc_lm_weight=WEIGHT))
    want = model_of(case, model.NgramScorer(WordModel(text), vocab, WEIGHT * math.log(10.0)), args.padding_idx)
    got = run_cli(sub, cli, "ngram", ["--hip_ctc_merge", "1", "--rank_model", "n-gram", "--rnnlm", path])
    assert got.decode("utf-8").splitlines() == lines_of(want, vocab, args)


def test_decode_asr_art_ctc_only_merged(tmp_path):
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.data.vocab import Vocab

    m, args, batch = ast("fp32")
    conf = dict(decode_type="ctc_only", ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0)
    scp, ckpt, cfg = _write_case(tmp_path, args, dict((k, v.detach().cpu().numpy()) for k, v in m.named_parameters()), batch[0].cpu().numpy(),
                                 [61, 57, 51], extra_conf=conf, ast=True)
    vocab = Vocab(str(tmp_path / "vocab.txt"), rank=1)
    cli = ["--task", "art", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "3", "--hip_precision", "fp32",
           "--load_data_workers", "0"]
    free, _ = search(m, args, batch, vocab, 0)
    _, case = search(m, args, batch, vocab, 1)
    got = run_cli(tmp_path, cli, "merged", ["--hip_ctc_merge", "1"])
    assert got.decode("utf-8").splitlines() == lines_of(model_of(case, None, args.padding_idx), vocab, args)
    first = run_cli(tmp_path, cli, "plain")
    assert first.decode("utf-8").splitlines() == lines_of(free, vocab, args) and run_cli(tmp_path, cli, "off", ["--hip_ctc_merge", "0"]) == first


def test_decode_asr_refuses_the_flag_where_it_would_be_ignored(tmp_path):
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.bin import decode_asr

    m, args, batch, vocab, cli = cassnat_cli(tmp_path, "ctc_only")
    state = dict((k, v.detach().cpu().numpy()) for k, v in m.named_parameters())
    for i, (over, names) in enumerate(((dict(decode_type="att_only"), "att_only"), (dict(decode_type="att_only", sample_num=4), "ESA"))):
        sub = tmp_path / ("run%d" % i)
        sub.mkdir()
        conf = dict(dict(sample_num=1, vocab_file=str(tmp_path / "pieces.txt"), ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0), **over)
        scp, ckpt, cfg = _write_case(sub, args, state, batch[0].cpu().numpy(), [61, 50, 37], extra_conf=conf)
        with pytest.raises(NotImplementedError, match="hip_ctc_merge") as e:
            decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "3",
                             "--hip_precision", "fp32", "--load_data_workers", "0", "--result_file", str(sub / "result.txt"), "--hip_ctc_merge", "1"])
        assert names in str(e.value)
