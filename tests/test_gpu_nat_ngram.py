"""CASS-NAT decoding with word n-gram shallow fusion in the finish loop (include/cassnat_hip_nat_ngram.h) end to end:
CassNAT.beam_decode with a models.ngram.NgramLM as lm_model on the tiny fixtures of tests/nat_lm_cases.py, against the numpy model
(tests/nat_ngram_model.py) run on the pass's own rows - fetched from the engine, so the beams are equal exactly at every precision -,
the attach / detach contract on real handles, and CassNATTask through decode_asr.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import nat_ngram_cases as cases
import nat_ngram_model as nn
from conftest import load_golden
from nat_lm_cases import CASES, TINY
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models import make_cassnat_model
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode

pytestmark = pytest.mark.gpu

V = 40
VOCAB = cases.vocab_of(V)


def load(model, state):
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[k]))
    return model


def build(name, prec):
    args, state, feats, sizes, _, _, extra = CASES[name]()
    assert args.vocab_size == V
    args.hip_precision, args.rank_model, args.hip_capture = prec, "n-gram", True
    if "select_seed" in extra:
        args.esa_select = load_golden(name)["select"]
    return args, load(make_cassnat_model(args.input_size, args).cuda(), state), feats, sizes, extra


def decode(model, args, feats, sizes, extra, lm):
    src = torch.from_numpy(feats).cuda()
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    size = torch.from_numpy(sizes).cuda()
    with torch.no_grad():
        top = ctc_beam_decode(model, src, mask, size, VOCAB, args, None) if extra.get("ctc_att") else None
        out, _ = model.beam_decode(src, mask, size, VOCAB, args, lm, top)
    return out


def model_beams(model, args, wm, scale, trace=None):
    """The numpy model on the rows the last pass left in the engine."""
    eng = model._engine
    att, ylen = np.asarray(eng.fetch("att_out"), np.float32), np.asarray(eng.fetch("ylen"))
    esa = getattr(args, "sample_num", 0) > 1
    ymax = int(ylen.max()) if esa else att.shape[1]
    return nn.finish(att, ylen, ymax, wm, VOCAB, cases.EOS, int(args.beam_width), scale, args.length_penalty, cases.SOS, args.padding_idx,
                     zero_past_len=esa, trace=trace)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", TINY)
def test_every_beam_is_the_model_on_the_pass_own_rows(name, prec):
    """att_only with and without the trigger mask, beam 1, ESA ranked by the same model, ctc_att, conformer blocks: hypotheses, their
    order and the float64 scores are the model's exactly; 'ys' has grown with the hypothesis; and the model decides something."""
    lm, wm = cases.plain_lm(V)
    args, model, feats, sizes, extra = build(name, prec)
    beams = decode(model, args, feats, sizes, extra, lm)
    scale = float(np.float32(float(args.lm_weight) * np.log(10.0)))
    trace = []
    want = model_beams(model, args, wm, scale, trace)
    cases.same_beams([[{"hyp": s["hyp"], "score": s["score"]} for s in u] for u in beams], want)
    for u in beams:
        assert len(u) == args.beam_width
        for s in u:
            assert isinstance(s["score"], float) and s["ys"].dtype == torch.long
            assert tuple(s["ys"].shape) == (1, len(s["hyp"])) and s["ys"][0].tolist() == s["hyp"] and s["hyp"][0] == cases.SOS
    free = model_beams(model, args, wm, 0.0)
    for b, (w, f) in enumerate(zip(want, free)):
        word = any(a[0] != 0 for bb, _, _, a in trace if bb == b)
        eos = any(a[1] != 0 for bb, _, _, a in trace if bb == b)
        assert w[0]["hyp"] != f[0]["hyp"] or (word and eos), b


def test_detached_the_engine_decodes_as_before_and_the_two_models_exclude_each_other():
    from cassnat_asr_public_amd.models.lm import make_model as make_lm

    lm, _ = cases.plain_lm(V)
    args, model, feats, sizes, extra = build("nat_lm_tiny", "fp32")
    _, _, _, _, lm_args, lm_state, _ = CASES["nat_lm_tiny"]()
    lm_args.hip_precision = "fp32"
    tlm = load(make_lm(lm_args).cuda(), lm_state)
    weight, args.lm_weight = args.lm_weight, 0
    before = decode(model, args, feats, sizes, extra, None)
    args.lm_weight = weight
    fused = decode(model, args, feats, sizes, extra, lm)
    with_tlm = decode(model, args, feats, sizes, extra, tlm)  # the TransformerLM finish on the same handle, after the detach
    g = load_golden("nat_lm_tiny")
    assert [s["hyp"] for s in with_tlm[0]] == [g["beam_hyp"][0, j, : g["beam_len"][0, j]].tolist() for j in range(3)]
    args.lm_weight = 0
    after = decode(model, args, feats, sizes, extra, lm)
    key = lambda out: [[(s["hyp"], s["score"]) for s in u] for u in out]  # noqa: E731
    assert key(before) == key(after) and key(before) != key(fused)
    # attached, each model refuses the other; a handle that is no CASS-NAT model refuses the n-gram model
    eng = model._engine
    lm.cuda()
    desc = lm.desc(lm.device)
    lm_eng = tlm.step_engine(3)
    eng.nat_attach_ngram(desc, 0.5)
    with pytest.raises(hip.HipError, match="n-gram model is attached"):
        eng.nat_attach_lm(lm_eng)
    eng.nat_attach_ngram(None)
    eng.nat_attach_lm(lm_eng)
    with pytest.raises(hip.HipError, match="TransformerLM is attached"):
        eng.nat_attach_ngram(desc, 0.5)
    eng.nat_attach_lm(None)
    with pytest.raises(hip.HipError, match="cfg.ast = 0"):
        lm_eng.nat_attach_ngram(desc, 0.5)

    def changed(**kw):
        d = hip.CnNgramDesc.from_buffer_copy(desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for d, scale, what in ((changed(order=0), 0.5, "order 0 is outside"), (changed(order=9), 0.5, "order 9 is outside"), (changed(vocab=41), 0.5, "vocabulary"),
                           (changed(word_slots=12), 0.5, "powers of two"), (changed(gram_bo=None), 0.5, "null table"), (desc, float("nan"), "must be a number")):
        with pytest.raises(hip.HipError, match=what):
            eng.nat_attach_ngram(d, scale)
    # nothing attached: the finish is an error, not a read of a stale model
    opts = hip.Engine.make_opts(args)
    hyp = torch.empty(3, 3, 20, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipError, match="cn_nat_attach_ngram"):
        eng.nat_ngram_finish(opts, 5, 3, cases.EOS, 0.1, False, hyp, torch.empty(3, 3, dtype=torch.int32, device="cuda"),
                             torch.empty(3, 3, dtype=torch.float64, device="cuda"))


def test_finish_needs_the_rows_of_the_pass():
    lm, _ = cases.plain_lm(V)
    args, model, feats, sizes, extra = build("nat_lm_tiny_bw1", "bf16")
    args.hip_capture, weight, args.lm_weight = False, args.lm_weight, 0
    decode(model, args, feats, sizes, extra, None)  # a greedy pass that kept the arg-max alone
    args.lm_weight = weight
    with pytest.raises(hip.HipError, match="kept no log-probability rows"):
        model._ngram_finish(model._engine, hip.Engine.make_opts(args), args, lm, 3, 5, False, VOCAB)


def test_decode_asr_cli_task_cassnat_with_an_arpa_file(tmp_path):
    """--lm_weight W --rank_model n-gram --rnnlm FILE.arpa: the result file holds the fused best beam per utterance, which differs from
    the LM-free one somewhere."""
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.data.vocab import Vocab
    from cassnat_asr_public_amd.tasks.cassnat_task import hyp_to_words
    from ngram_model import random_arpa

    args, state, feats, sizes, _, _, extra = CASES["nat_lm_tiny"]()
    scp, ckpt, cfg = _write_case(tmp_path, args, state, feats, [61, 50, 37])
    (tmp_path / "vocab.txt").write_text("".join(VOCAB.index2word[i] + "\n" for i in range(4, V)), encoding="utf-8")
    vocab = Vocab(str(tmp_path / "vocab.txt"), rank=1)
    assert vocab.n_words == V and vocab.index2word == VOCAB.index2word
    arpa = tmp_path / "model.arpa"
    arpa.write_text(random_arpa(cases.WORDS, 3, seed=6), encoding="utf-8")
    result = str(tmp_path / "token_results.txt")
    rc = decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                          "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0", "--lm_weight", "0.6",
                          "--rnnlm", str(arpa), "--rank_model", "n-gram"])
    assert rc == 0
    lm, _ = cases.plain_lm(V)  # (the same text)
    args2, model, feats, sizes, extra = build("nat_lm_tiny", "fp32")
    fused = decode(model, args2, feats, sizes, extra, lm)
    args2.lm_weight = 0
    free = decode(model, args2, feats, sizes, extra, None)
    lines = lambda out: ["spk-utt%02d " % b + " ".join(hyp_to_words(u[0]["hyp"], vocab, args.padding_idx)) for b, u in enumerate(out)]  # noqa: E731
    assert open(result, encoding="utf-8").read().splitlines() == lines(fused)
    assert lines(fused) != lines(free)
