"""AST beam search with contextual phrase biasing (include/cassnat_hip_ast_bias.h) through Transformer.beam_decode: the device loop
(cn_decode_ast with a list attached, its nodes carried from step to step) against the host-bookkeeping loop (cn_ast_step_bias) run
with a test-owned object whose ``ast_nodes_host`` / ``ast_terms_host`` are the numpy model of tests/ast_bias_model.py, which rescans
every hypothesis from its first token - every beam's hypothesis, order and score bit for bit - over CTC weights, beam widths, length
penalties, the transformer and conformer AST and the engines.  The lists are cut from the run itself: a pair of neighbouring pieces
of an unbiased lower beam that the best beam lacks (one piece where no beam offers two), with the smallest score of 1, 2, 4 .. 32 that makes a hypothesis holding it the
best.  Then the detach, the empty list, the refusals beside an n-gram model and a TransformerLM, and decode_asr --task art with
--hip_bias FILE --hip_bias_search att.

Two configurations cannot show "the best hypothesis changes", as in tests/test_gpu_ast_ngram.py: with CTC at beams (1, 1) the one
candidate is the attention's best, which the terms are added to and cannot replace; with CTC at (28, 28) the whole vocabulary is the
candidate list and the CTC prefix scorer makes [sos, blank, eos] every best.  There the list is cut and judged one beam lower
(28, 28), respectively taken from the (3, 5) run and only the equality of the two loops is asserted (1, 1)."""
import copy
import functools

import numpy as np
import pytest
import torch

import ast_bias_cases as cases
import ast_bias_model as model
from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models.bias import BiasList
from test_gpu_ast_ngram import BEAMS, EOS_BIAS, GAIN, LENGTHS, SEED, START_BIAS, VOCAB, ast, same_beams

pytestmark = pytest.mark.gpu

assert BEAMS == [(1, 1), (3, 5), (10, 15), (28, 28)] and LENGTHS == [61, 50, 37] and VOCAB.n_words == cases.V


class ModelBias(object):
    """What the host loop asks of a phrase list, answered by the numpy model from the token rows alone; the tables the device needs
    are the BiasList's."""

    def __init__(self, bias):
        self.bias, self.phrases, self.rows_seen, self.terms_seen = bias, dict(bias.phrases), 0, 0

    def cuda(self, device=None):
        self.bias.cuda(device)
        return self

    def desc(self, where="host"):
        return self.bias.desc(where)

    def ast_nodes_host(self, rows, lens):
        self.rows_seen += len(rows)
        return np.array([model.node_id(self.bias, model.node(rows[r, :lens[r]].tolist(), self.phrases)) for r in range(len(rows))], np.int32)

    def ast_terms_host(self, nodes, idx, eos):
        # (the open match is all of a hypothesis that a term depends on: the node's own pieces stand for the hypothesis)
        self.terms_seen += idx.size
        return np.array([model.terms(list(model.node_of_id(self.bias, int(n))), self.phrases, eos, 2 ** 31 - 1, idx[k])
                         for k, n in enumerate(nodes)], np.float32).reshape(idx.shape)


def decode(preset, prec, bias=None, host_beam=False, fresh=0, **over):
    base, net, src = ast(preset, prec, fresh)
    args = copy.copy(base)
    args.hip_host_beam, args.lm_weight = host_beam, 0
    for k, v in over.items():
        setattr(args, k, v)
    with torch.no_grad():
        return net.beam_decode(src, (src[:, :, 0] != args.padding_idx).unsqueeze(1), VOCAB, args, None, bias=bias)


def pairs(hyp):
    """The spans of two neighbouring pieces and of one piece behind sos."""
    return set(zip(hyp[1:], hyp[2:])) | {(t,) for t in hyp[1:]}


def lacking_pair(utt, top):
    """Two neighbouring pieces (no special id: a list file cannot name those) of a beam below beam ``top`` that beam ``top`` lacks;
    where no beam offers two, one piece."""
    have = pairs(utt[top]["hyp"])
    for n in (2, 1):
        for s in utt[top + 1:]:
            h = s["hyp"][1:]
            for span in zip(*(h[i:] for i in range(n))):
                if min(span) >= 4 and span not in have:
                    return span
    return None


@functools.lru_cache(maxsize=None)
def winning_list(preset, prec, ctc_weight, bw, K, lp):
    """({pair: score}, utterance, the beam that is judged): cut from the unbiased run of the same configuration."""
    top = 1 if ctc_weight > 0 and K == cases.V else 0
    cut = dict(beam_width=3, ctc_beam=5) if bw == 1 else dict(beam_width=bw, ctc_beam=K)
    free = decode(preset, prec, None, ctc_weight=ctc_weight, length_penalty=lp, **cut)
    found = [(b, lacking_pair(u, top)) for b, u in enumerate(free) if len(u) > top + 1 and lacking_pair(u, top)]
    assert found, "no utterance has a lower beam with a pair of pieces that its best beam lacks"
    b, pair = found[0]
    for score in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0):
        out = decode(preset, prec, BiasList.from_phrases({pair: score}), ctc_weight=ctc_weight, length_penalty=lp, **cut)
        if pair in pairs(out[b][top]["hyp"]):
            return {pair: score}, b, top
    raise AssertionError("no score up to 32 makes a hypothesis with the pair %r the best" % (pair,))


def check_config(preset, prec, phrases, **over):
    """Device loop == host loop with the numpy model's nodes and terms, bit for bit."""
    bias = BiasList.from_phrases(phrases)
    owned = ModelBias(bias)
    dev_b = decode(preset, prec, bias, **over)
    host_b = decode(preset, prec, owned, host_beam=True, **over)
    assert owned.rows_seen > 0 and (owned.terms_seen > 0) == (over["ctc_weight"] > 0)
    same_beams(dev_b, host_b)
    return dev_b, decode(preset, prec, None, **over)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("bw,K", BEAMS)
@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_device_loop_is_the_host_loop_with_the_model(ctc_weight, bw, K, prec):
    for lp in (None, 0.5):
        phrases, b, top = winning_list("tiny_ast", prec, ctc_weight, bw, K, lp)
        (pair, score), = phrases.items()
        dev_b, free = check_config("tiny_ast", prec, phrases, ctc_weight=ctc_weight, beam_width=bw, ctc_beam=K, length_penalty=lp)
        held = [pair in pairs(s["hyp"]) for s in dev_b[b]]
        print(f"ast bias {prec} ctc {ctc_weight} beams {bw}/{K} lp {lp}: pair {pair} score {score} utterance {b}, held by beams {held}")
        if bw == 1:
            continue  # (the list is the (3, 5) run's: only the two loops' equality is claimed)
        # the beam that lacked the pair gave way to one that holds it
        assert pair in pairs(dev_b[b][top]["hyp"]) and pair not in pairs(free[b][top]["hyp"])
        assert dev_b[b][top]["hyp"] != free[b][top]["hyp"]
        if top == 1:
            assert all(u[0]["hyp"] == [cases.SOS, cases.BLANK, cases.EOS] for u in dev_b)
        assert any(s["hyp"][-1] == cases.EOS for u in dev_b for s in u), "no hypothesis ended with eos"


@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_conformer_ast(ctc_weight):
    phrases, b, top = winning_list("tiny_conf_ast", "fp32", ctc_weight, 10, 15, 0.5)
    dev_b, free = check_config("tiny_conf_ast", "fp32", phrases, ctc_weight=ctc_weight, beam_width=10, ctc_beam=15, length_penalty=0.5)
    assert dev_b[b][0]["hyp"] != free[b][0]["hyp"] and next(iter(phrases)) in pairs(dev_b[b][0]["hyp"])


def richer_list(free):
    """Phrases cut from the unbiased beams: spans of 2 to 4 pieces of every beam, scores 2 / 0.5 / -1 / 1.37 in turn (the last is not
    dyadic: every operation of the fusion is still a defined one), spans that share prefixes and overlap, so that failure links,
    banks and break-offs all occur."""
    out, scores = {}, (2.0, 0.5, -1.0, 1.37)
    for u in free:
        for s in u:
            h = [t for t in s["hyp"][1:] if t >= 4]
            for i in range(0, max(0, len(h) - 1), 3):
                ids = tuple(h[i:i + 2 + (i // 3) % 3])
                if len(ids) >= 2:
                    out.setdefault(ids, scores[len(out) % 4])
    assert len(out) >= 6
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_a_list_of_many_overlapping_phrases_is_still_bit_exact(ctc_weight, prec):
    over = dict(ctc_weight=ctc_weight, beam_width=10, ctc_beam=15, length_penalty=0.5)
    phrases = richer_list(decode("tiny_ast", prec, None, **over))
    dev_b, free = check_config("tiny_ast", prec, phrases, **over)
    assert any([s["hyp"] for s in u] != [s["hyp"] for s in v] for u, v in zip(dev_b, free))
    banks = sum(model.segment(s["hyp"][1:], phrases) != [t for t in s["hyp"][1:]] for u in dev_b for s in u)
    assert banks > 0  # phrases were completed


@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_after_a_detach_the_handle_decodes_as_if_nothing_had_been_attached(ctc_weight):
    over = dict(ctc_weight=ctc_weight, beam_width=3, ctc_beam=5, length_penalty=0.5)
    phrases, b, _ = winning_list("tiny_ast", "fp32", ctc_weight, 3, 5, 0.5)
    fused = decode("tiny_ast", "fp32", BiasList.from_phrases(phrases), **over)
    after = decode("tiny_ast", "fp32", None, **over)
    never = decode("tiny_ast", "fp32", None, fresh=1, **over)
    assert ast("tiny_ast", "fp32")[1] is not ast("tiny_ast", "fp32", 1)[1]
    same_beams(after, never)
    assert fused[b][0]["hyp"] != after[b][0]["hyp"]


@pytest.mark.parametrize("host_beam", [False, True])
@pytest.mark.parametrize("ctc_weight", [0.3, 0])
def test_the_empty_list_is_no_list(ctc_weight, host_beam):
    over = dict(ctc_weight=ctc_weight, beam_width=3, ctc_beam=5, length_penalty=0.5)
    empty = BiasList.from_phrases({})
    assert empty.nodes == 1
    same_beams(decode("tiny_ast", "fp32", empty, host_beam=host_beam, **over), decode("tiny_ast", "fp32", None, **over))


@pytest.mark.parametrize("host_beam", [False, True])
def test_a_list_beside_an_ngram_model_or_a_transformer_lm_is_refused(host_beam):
    from ast_ngram_cases import lm_of
    from cassnat_asr_public_amd.models.lm import make_model as make_lm

    base, net, src = ast("tiny_ast", "fp32")
    args = copy.copy(base)
    args.hip_host_beam, args.beam_width, args.ctc_beam = host_beam, 3, 5
    bias = cases.bias_of("shared_prefix")
    dev = src.device
    bias.cuda(dev)
    eng = net.engine(3, 61)
    # an n-gram model: whichever comes second is refused by name
    lm, _ = lm_of(3)
    lm.cuda(dev)
    try:
        eng.ast_attach_ngram(lm.desc(dev), 0.5)
        with pytest.raises(hip.HipError, match="cn_ast_attach_bias: an n-gram model is attached"):
            eng.ast_attach_bias(bias.desc(dev))
        eng.ast_attach_ngram(None)
        eng.ast_attach_bias(bias.desc(dev))
        with pytest.raises(hip.HipError, match="cn_ast_attach_ngram: a phrase list is attached"):
            eng.ast_attach_ngram(lm.desc(dev), 0.5)
    finally:
        eng.ast_attach_ngram(None)
        eng.ast_attach_bias(None)
    # a TransformerLM: the search refuses, in both loops
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=cases.V)
    lm_args.hip_precision = "fp32"
    tlm = make_lm(lm_args).cuda()
    opts = hip.CnDecodeOpts(padding_idx=0, sos=cases.SOS, beam_width=1)
    try:
        eng.ast_attach_lm(tlm.step_engine(3 * 3))
        eng.ast_attach_bias(bias.desc(dev))
        for lm_weight, holder in ((0.6, None), (0.0, bias)):  # the LM's step, then the list's step, each beside the other
            with pytest.raises(hip.HipError, match="cannot be fused together|attached together"):
                net._beam_search(eng, src, opts, args, cases.SOS, cases.EOS, 3, 5, True, 8, lm_weight, dev, None, 0.0, holder)
    finally:
        eng.ast_attach_lm(None)
        eng.ast_attach_bias(None)
    # and beam_decode refuses the pair before it touches the device
    args.lm_weight = 0.5
    with pytest.raises(NotImplementedError, match="hip_bias"):
        net.beam_decode(src, None, VOCAB, args, tlm, bias=bias)


def test_decode_asr_cli_task_art_with_a_list(tmp_path):
    """decode_asr --task art --hip_bias F --hip_bias_search att writes the file the host loop with the model gives; without the new
    flag the list is refused as before; without --hip_bias the file is the unbiased decode's."""
    import yaml

    import ast_ngram_model
    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.data import kaldi_io
    from cassnat_asr_public_amd.data.vocab import Vocab
    from cassnat_asr_public_amd.tasks.cassnat_task import hyp_to_words

    base, _, src = ast("tiny_ast", "fp32")
    args = copy.copy(base)
    args.beam_width, args.ctc_beam, args.length_penalty = 3, 5, 0.5
    state = synth.make_state(args, seed=SEED, gain=GAIN)
    state["att_generator.proj.bias"][cases.EOS] += EOS_BIAS
    state["att_generator.proj.bias"][ast_ngram_model.starts_of(cases.VOCAB) != 0] += START_BIAS
    feats = src.cpu().numpy()
    scp = str(tmp_path / "feats.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "feats.ark"), scp, [(f"spk-utt{b}", feats[b, :n]) for b, n in enumerate(LENGTHS)])
    vocab_file = tmp_path / "pieces.txt"
    vocab_file.write_text("".join(cases.VOCAB.index2word[i] + "\n" for i in range(4, cases.V)), encoding="utf-8")
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight", "max_decode_ratio",
                                          "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(vocab_file=str(vocab_file), use_gpu=True, n_features=80, model_type="transformer")
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))
    vocab = Vocab(str(vocab_file), rank=1)
    assert [vocab.index2word[i] for i in range(cases.V)] == [cases.VOCAB.index2word[i] for i in range(cases.V)]
    over = dict(ctc_weight=args.ctc_weight, beam_width=3, ctc_beam=5, length_penalty=0.5)
    phrases, b, _ = winning_list("tiny_ast", "fp32", args.ctc_weight, 3, 5, 0.5)
    (pair, score), = phrases.items()
    listed = tmp_path / "bias.txt"
    listed.write_text("# cut from a lower beam\n\n%s\n" % " ".join(vocab.index2word[i] for i in pair), encoding="utf-8")

    def run(tag, flags):
        result = str(tmp_path / ("result_%s.txt" % tag))
        rc = decode_asr.main(["--task", "art", "--test_config", str(cfg), "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                              "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0"] + flags)
        assert rc == 0
        return open(result, "rb").read()

    def lines(recog):
        return [f"spk-utt{k} " + " ".join(hyp_to_words(seqs[0]["hyp"], vocab, args.padding_idx)) for k, seqs in enumerate(recog)]

    host = decode("tiny_ast", "fp32", ModelBias(BiasList.from_phrases(phrases)), host_beam=True, **over)
    free = decode("tiny_ast", "fp32", None, **over)
    assert host[b][0]["hyp"] != free[b][0]["hyp"]
    biased = run("bias", ["--hip_bias", str(listed), "--hip_bias_score", repr(score), "--hip_bias_search", "att"])
    assert biased.decode("utf-8").splitlines() == lines(host)
    with pytest.raises(NotImplementedError, match="hip_bias biases the CTC prefix beam search"):
        run("refused", ["--hip_bias", str(listed)])
    plain = run("plain", [])
    assert plain.decode("utf-8").splitlines() == lines(free) and plain != biased
    assert run("plain2", ["--hip_bias_search", "att"]) == plain  # (the flag alone names a search, it biases nothing)
