"""AST beam search with word n-gram shallow fusion (include/cassnat_hip_ast_ngram.h) through Transformer.beam_decode: the device
loop (cn_decode_ast with a model attached) against the host-bookkeeping loop (cn_ast_step_ngram) run with a test-owned object whose
``ast_adds_host`` is the numpy model of tests/ast_ngram_model.py - every beam's hypothesis, order and score bit for bit - over
CTC weights, beam widths, length penalties, model orders and engines; the detach, the refusal of two LM kinds at once, and
decode_asr --task art with --rank_model n-gram and an ARPA file."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import ast_ngram_cases as cases
import ast_ngram_model as model_of
from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models import make_conformer, make_transformer
from cassnat_asr_public_amd.models.ngram import NgramLM
from ctc_ngram_model import WordModel
from ngram_model import random_arpa
from types import SimpleNamespace

pytestmark = pytest.mark.gpu

VOCAB = SimpleNamespace(word2index=dict(cases.IX), index2word=cases.VOCAB.index2word, n_words=cases.V)
LM_WEIGHT = 0.5 / math.log(10.0)  # float32(lm_weight * ln 10) is 0.5: with the dyadic models every fused term is exact
# Seed and biases (added to the attention generator's bias: random weights end few hypotheses and begin few words) were picked so
# that every configuration below meets its facts on all three engines: seeds 1 .. 20 were tried, three met them.
SEED, GAIN = 10, 2.0
EOS_BIAS, START_BIAS = 3.0, 1.5
LENGTHS = [61, 50, 37]
BEAMS = [(1, 1), (3, 5), (10, 15), (28, 28)]


def test_the_weight_gives_the_scale_one_half():
    assert np.float32(LM_WEIGHT * math.log(10.0)) == np.float32(0.5)


class ModelAdds(object):
    """What the host loop asks of an n-gram model, answered by the numpy model; the tables the device needs are the NgramLM's."""

    def __init__(self, lm, model):
        self.lm, self.model, self.device_ok, self.rows_seen = lm, model, True, 0

    def cuda(self, device=None):
        self.lm.cuda(device)
        return self

    def desc(self, where="host"):
        return self.lm.desc(where)

    def ast_adds_host(self, rows, lens, eos):
        self.rows_seen += len(rows)
        return np.array([model_of.adds(self.model, cases.VOCAB, rows[r, :lens[r]].tolist(), eos) for r in range(len(rows))], np.float32)


@functools.lru_cache(maxsize=None)
def ast(preset, prec, fresh=0):
    """(args, model, feats) of the tiny AST model over the 28 pieces; ``fresh``: another instance with the same weights."""
    args = synth.make_args_ast(preset, vocab_size=cases.V, max_decode_ratio=1.0)
    args.hip_precision = prec
    state = synth.make_state(args, seed=SEED, gain=GAIN)
    bias = state["att_generator.proj.bias"]
    bias[cases.EOS] += EOS_BIAS
    bias[model_of.starts_of(cases.VOCAB) != 0] += START_BIAS
    make = make_conformer if getattr(args, "model_type", "transformer") == "conformer" else make_transformer
    model = make(args.input_size, args).cuda()
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[k]))
    feats, _ = synth.make_feats(3, 61, 80, lengths=LENGTHS, seed=11)
    return args, model, torch.from_numpy(feats).cuda()


def decode(preset, prec, lm_model=None, host_beam=False, fresh=0, **over):
    base, model, src = ast(preset, prec, fresh)
    args = copy.copy(base)
    args.hip_host_beam = host_beam
    args.lm_weight = LM_WEIGHT
    for k, v in over.items():
        setattr(args, k, v)
    if lm_model is None:
        args.lm_weight = 0
    with torch.no_grad():
        return model.beam_decode(src, (src[:, :, 0] != args.padding_idx).unsqueeze(1), VOCAB, args, lm_model)


def same_beams(got, want):
    assert len(got) == len(want)
    for b, (u, v) in enumerate(zip(got, want)):
        assert [s["hyp"] for s in u] == [s["hyp"] for s in v], b
        assert [s["score"] for s in u] == [s["score"] for s in v], b


def check_config(preset, prec, lm, model, **over):
    """Device loop == host loop with the numpy model's adds, bit for bit; and the model decides something."""
    owned = ModelAdds(lm, model)
    dev_b = decode(preset, prec, lm, **over)
    host_b = decode(preset, prec, owned, host_beam=True, **over)
    assert owned.rows_seen > 0
    same_beams(dev_b, host_b)
    free = decode(preset, prec, None, **over)
    hyps = [s["hyp"] for u in dev_b for s in u]
    facts = dict(differs=any(u[0]["hyp"] != v[0]["hyp"] for u, v in zip(dev_b, free)),
                 two_words=any(len(model_of.closed_words(model, cases.VOCAB, h[1:], cases.EOS)) >= 2 for h in hyps),
                 ended=any(h[-1] == cases.EOS for h in hyps),
                 rescored=any(u[0]["score"] != v[0]["score"] for u, v in zip(dev_b, free)),
                 beams_differ=any([s["hyp"] for s in u] != [s["hyp"] for s in v] for u, v in zip(dev_b, free)))
    return dev_b, facts


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("bw,K", BEAMS)
@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_device_loop_is_the_host_loop_with_the_model(ctc_weight, bw, K, prec):
    for order in (2, 3):
        lm, model = cases.lm_of(order)
        for lp in (None, 0.5):
            dev_b, facts = check_config("tiny_ast", prec, lm, model, ctc_weight=ctc_weight, beam_width=bw, ctc_beam=K, length_penalty=lp)
            print(f"ast n-gram {prec} ctc {ctc_weight} beams {bw}/{K} lp {lp} order {order}: {facts}")
            if ctc_weight > 0 and K == 1:
                # one slot and one candidate, the attention's best, which the terms are added to but cannot replace: the hypotheses
                # are the LM-free ones by construction, and what the model changes is their score
                assert not facts["differs"] and facts["rescored"]
            elif ctc_weight > 0 and K == cases.V:
                # the whole vocabulary is the candidate list, blank among it: the CTC prefix scorer lifts [sos, blank, eos] above
                # everything by 1e10 with or without a model (float32 absorbs the rest: its score is 0.0), so every utterance's best
                # is that hypothesis by construction; the model shows in the beams below it
                assert all(u[0]["hyp"] == [cases.SOS, cases.BLANK, cases.EOS] for u in dev_b)
                assert facts["beams_differ"], "no utterance's beams differ from the LM-free decode"
            else:
                assert facts["differs"], "no utterance's best hypothesis differs from the LM-free decode"
            assert facts["two_words"], "no hypothesis closed two words"
            assert facts["ended"], "no hypothesis ended with eos"


@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_conformer_ast(ctc_weight):
    lm, model = cases.lm_of(3)
    _, facts = check_config("tiny_conf_ast", "fp32", lm, model, ctc_weight=ctc_weight, beam_width=3, ctc_beam=5, length_penalty=0.5)
    assert facts["differs"]


@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_a_model_that_is_not_dyadic_is_still_bit_exact(tmp_path, ctc_weight):
    """Every operation of the fusion is a defined float32 one, so the two loops agree whatever the values."""
    text = random_arpa(cases.WORDS, 3, seed=21)
    path = tmp_path / "random.arpa"
    path.write_text(text, encoding="utf-8")
    lm = NgramLM.load(str(path), cases.VOCAB)
    _, facts = check_config("tiny_ast", "fp32", lm, WordModel(text), ctc_weight=ctc_weight, beam_width=10, ctc_beam=15, length_penalty=0.5,
                            lm_weight=0.37)
    assert facts["differs"]


@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_after_a_detach_the_handle_decodes_as_if_nothing_had_been_attached(ctc_weight):
    lm, _ = cases.lm_of(3)
    over = dict(ctc_weight=ctc_weight, beam_width=3, ctc_beam=5, length_penalty=0.5)
    fused = decode("tiny_ast", "fp32", lm, **over)
    after = decode("tiny_ast", "fp32", None, **over)
    never = decode("tiny_ast", "fp32", None, fresh=1, **over)
    assert ast("tiny_ast", "fp32")[1] is not ast("tiny_ast", "fp32", 1)[1]
    same_beams(after, never)
    assert any(u[0]["hyp"] != v[0]["hyp"] for u, v in zip(fused, after))


@pytest.mark.parametrize("host_beam", [False, True])
def test_an_ngram_model_and_a_transformer_lm_together_are_refused(host_beam):
    from cassnat_asr_public_amd.models.lm import make_model as make_lm

    lm, _ = cases.lm_of(3)
    base, model, src = ast("tiny_ast", "fp32")
    args = copy.copy(base)
    args.hip_host_beam, args.beam_width, args.ctc_beam = host_beam, 3, 5
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=cases.V)
    lm_args.hip_precision = "fp32"
    tlm = make_lm(lm_args).cuda()
    eng = model.engine(3, 61)
    dev = src.device
    lm.cuda(dev)
    eng.ast_attach_lm(tlm.step_engine(3 * 3))
    eng.ast_attach_ngram(lm.desc(dev), 0.5)
    opts = hip.CnDecodeOpts(padding_idx=0, sos=cases.SOS, beam_width=1)
    try:
        with pytest.raises(hip.HipError, match="cannot be fused together"):
            model._beam_search(eng, src, opts, args, cases.SOS, cases.EOS, 3, 5, True, 8, 0.6, dev)
    finally:
        eng.ast_attach_lm(None)
        eng.ast_attach_ngram(None)
    # a vocabulary whose pieces cannot be glued is refused before anything is attached
    bad = ModelAdds(lm, None)
    bad.device_ok = False
    with pytest.raises(ValueError, match="separator behind its leading run"):
        decode("tiny_ast", "fp32", bad)


def test_decode_asr_cli_task_art_with_an_arpa_file(tmp_path):
    """decode_asr --task art --lm_weight W --rank_model n-gram --rnnlm model.arpa writes the file the host loop gives."""
    import yaml

    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.data import kaldi_io
    from cassnat_asr_public_amd.data.vocab import Vocab
    from cassnat_asr_public_amd.tasks.cassnat_task import hyp_to_words
    from ctc_ngram_model import dyadic_arpa

    base, _, src = ast("tiny_ast", "fp32")
    args = copy.copy(base)
    args.beam_width, args.ctc_beam, args.length_penalty = 3, 5, 0.5
    state = synth.make_state(args, seed=SEED, gain=GAIN)
    state["att_generator.proj.bias"][cases.EOS] += EOS_BIAS
    state["att_generator.proj.bias"][model_of.starts_of(cases.VOCAB) != 0] += START_BIAS
    feats = src.cpu().numpy()
    scp = str(tmp_path / "feats.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "feats.ark"), scp, [(f"spk-utt{b}", feats[b, :n]) for b, n in enumerate(LENGTHS)])
    vocab_file = tmp_path / "pieces.txt"
    vocab_file.write_text("".join(cases.VOCAB.index2word[i] + "\n" for i in range(4, cases.V)), encoding="utf-8")
    arpa = tmp_path / "model.arpa"
    arpa.write_text(dyadic_arpa(cases.WORDS, 3, seed=3), encoding="utf-8")
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight", "max_decode_ratio",
                                          "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(vocab_file=str(vocab_file), use_gpu=True, n_features=80, model_type="transformer")
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))
    result = str(tmp_path / "token_results.txt")
    rc = decode_asr.main(["--task", "art", "--test_config", str(cfg), "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                          "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0", "--lm_weight", "0.5",
                          "--rank_model", "n-gram", "--rnnlm", str(arpa)])
    assert rc == 0
    vocab = Vocab(str(vocab_file), rank=1)
    assert [vocab.index2word[i] for i in range(cases.V)] == [cases.VOCAB.index2word[i] for i in range(cases.V)]
    lm = NgramLM.load(str(arpa), vocab)
    host = decode("tiny_ast", "fp32", lm, host_beam=True, beam_width=3, ctc_beam=5, length_penalty=0.5, lm_weight=0.5)
    free = decode("tiny_ast", "fp32", None, beam_width=3, ctc_beam=5, length_penalty=0.5)
    expect = [f"spk-utt{b} " + " ".join(hyp_to_words(seqs[0]["hyp"], vocab, args.padding_idx)) for b, seqs in enumerate(host)]
    assert open(result).read().splitlines() == expect
    assert any(u[0]["hyp"] != v[0]["hyp"] for u, v in zip(host, free))
