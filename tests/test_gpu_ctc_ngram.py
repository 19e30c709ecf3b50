"""CTC prefix beam search with word n-gram fusion end to end on the tiny model (d_model 128, vocabulary 40: the n-gram tests' pieces
padded to 40): ctc_beam_decode with an NgramLM against tests/ctc_ngram_model.py run on the engine's own log-posteriors, the invariant
score_lm = lm_scale * (the ranker's score of the hypothesis), a weight that changes the best hypothesis, ctc_att on the fused beams,
and decode_asr.py as a child process with --rank_model n-gram --rnnlm FILE.arpa."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import tiny_case
from cassnat_asr_public_amd.models.ngram import NgramLM
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode
from ctc_ngram_model import WordModel, dyadic_arpa, search
from ngram_model import text_of
from test_gpu_ctcbeam import build
from test_gpu_ngram import PIECES, WORDS

pytestmark = pytest.mark.gpu

PIECES40 = PIECES + ["▁x%d" % i for i in range(40 - len(PIECES))]
VOCAB = SimpleNamespace(index2word=dict(enumerate(PIECES40)), n_words=40, word2index={p: i for i, p in enumerate(PIECES40)})
WEIGHT = 0.3


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    text = dyadic_arpa(WORDS, 3, seed=3)
    path = tmp_path_factory.mktemp("ctc_ngram") / "model.arpa"
    path.write_text(text, encoding="utf-8")
    return str(path), text


def decode(prec, lm, weight=WEIGHT, capture=False, **kw):
    args, state, feats, sizes = tiny_case(decode_type="ctc_only", ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=weight,
                                          rank_model="n-gram", **kw)
    assert args.vocab_size == 40
    model = build(args, state, prec, capture=capture)
    src = torch.from_numpy(feats).cuda()
    mask, ratio = (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(sizes).cuda()
    with torch.no_grad():
        top = ctc_beam_decode(model, src, mask, ratio, VOCAB, args, lm)
    return top, model, args, (src, mask, ratio)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_the_search_equals_the_model_on_the_engines_own_log_posteriors(arpa, prec):
    path, text = arpa
    lm = NgramLM.load(path, VOCAB)
    top, model, args, (src, mask, ratio) = decode(prec, lm, capture=True)
    ctc_dev = model._engine.fetch("ctc_out")
    Tp = ctc_dev.shape[1]
    pruned = torch.topk(torch.from_numpy(np.asarray(ctc_dev, np.float32)), args.ctc_pruning, dim=-1)[1].numpy()
    sizes = [int(np.float32(r) * np.float32(Tp)) for r in ratio.cpu().numpy()]
    lm_scale = WEIGHT * math.log(10.0)
    ref = WordModel(text)
    want = search(ctc_dev, pruned, sizes, args.ctc_beam, args.ctc_lp, lm_scale, ref, VOCAB)
    assert len(top) == len(want) == 3
    for b, utt in enumerate(top):
        assert [s["hyp"] for s in utt] == [s["hyp"] for s in want[b]], b
        for key in ("score_ctc", "score_lm", "p_blk", "p_nblk"):
            np.testing.assert_allclose([s[key] for s in utt], [s[key] for s in want[b]], rtol=0, atol=1e-8, err_msg=key)
        for s in utt:
            assert s["ys"].dtype == torch.long and s["ys"][0].tolist() == [1] + s["hyp"]
    # the invariant: score_lm is lm_scale times the sum of the word scores the ranker adds for the hypothesis
    words = 0
    for utt in top:
        n = max(len(s["hyp"]) for s in utt)
        tok = np.zeros((len(utt), max(n, 1)), np.int32)
        for j, s in enumerate(utt):
            tok[j, :len(s["hyp"])] = s["hyp"]
        ylen = np.array([len(s["hyp"]) for s in utt], np.int32)
        host = lm.score_tokens_host(tok, ylen)
        for j, s in enumerate(utt):
            t = text_of(s["hyp"], len(s["hyp"]), VOCAB)
            assert abs(s["score_lm"] - lm_scale * float(host[j])) <= lm_scale * ref.bound(t) + 1e-12 * abs(s["score_lm"]), (s, t)
            words += len(t.split())
    assert words > 0


def test_a_large_weight_changes_the_best_hypothesis(arpa):
    path, _ = arpa
    lm = NgramLM.load(path, VOCAB)
    free, _, _, _ = decode("fp32", None, weight=0)
    zero, _, _, _ = decode("fp32", lm, weight=0)
    fused, _, _, _ = decode("fp32", lm, weight=2.0)
    key = lambda top: [[(s["hyp"], s["score_ctc"], s["score_lm"]) for s in u] for u in top]
    assert key(free) == key(zero) and all(s["score_lm"] == 0.0 for u in free for s in u)
    assert any(a[0]["hyp"] != b[0]["hyp"] for a, b in zip(free, fused)), [u[0]["hyp"] for u in free]
    assert all(s["score_lm"] < 0.0 for u in fused for s in u)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_ctc_att_runs_on_the_fused_beams(arpa, prec):
    path, _ = arpa
    lm = NgramLM.load(path, VOCAB)
    top, model, args, (src, mask, ratio) = decode(prec, lm)
    args.decode_type = "ctc_att"
    with torch.no_grad():
        out, _ = model.beam_decode(src, mask, ratio, VOCAB, args, lm, top)
        forced, _ = model.beam_decode(src, mask, ratio, VOCAB, args, None, [[{"hyp": list(u[0]["hyp"]), "ys": u[0]["ys"].clone()}] for u in top])
    assert len(out) == 3
    for a, b in zip(out, forced):
        assert a[0]["hyp"] == b[0]["hyp"] and a[0]["score"] == b[0]["score"]


@pytest.mark.parametrize("decode_type", ["ctc_only", "ctc_att"])
def test_decode_asr_child_process_with_an_arpa_file(tmp_path, arpa, decode_type):
    from test_gpu_multirank import _run_cli, _write_case
    from cassnat_asr_public_amd.data.vocab import Vocab
    from cassnat_asr_public_amd.tasks.cassnat_task import hyp_to_words

    path, _ = arpa
    args, state, feats, sizes = tiny_case(decode_type=decode_type, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=WEIGHT, rank_model="n-gram")
    vocab_file = tmp_path / "pieces.txt"
    vocab_file.write_text("".join(p + "\n" for p in PIECES40[4:]), encoding="utf-8")
    conf = dict(decode_type=decode_type, sample_num=1, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=WEIGHT, vocab_file=str(vocab_file))
    scp, ckpt, cfg = _write_case(tmp_path, args, state, feats, [61, 50, 37], extra_conf=conf)
    cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "3", "--hip_precision", "fp32",
           "--load_data_workers", "0", "--rank_model", "n-gram", "--rnnlm", path]
    lines = _run_cli(tmp_path, cli, 1, "nccl", decode_type)
    vocab = Vocab(str(vocab_file), rank=1)
    assert vocab.n_words == 40 and [vocab.index2word[i] for i in range(40)] == PIECES40
    lm = NgramLM.load(path, vocab)
    model = build(args, state, "fp32")
    src = torch.from_numpy(feats).cuda()
    mask, ratio = (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(sizes).cuda()
    with torch.no_grad():
        recog = ctc_beam_decode(model, src, mask, ratio, vocab, args, lm)
        if decode_type == "ctc_att":
            recog, _ = model.beam_decode(src, mask, ratio, vocab, args, lm, recog)
    expect = ["spk-utt%02d " % b + " ".join(hyp_to_words(seqs[0]["hyp"], vocab, args.padding_idx)) for b, seqs in enumerate(recog)]
    assert lines == expect
    assert any(len(l.split()) > 1 for l in lines)
