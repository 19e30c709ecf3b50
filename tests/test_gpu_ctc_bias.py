"""CTC prefix beam search with phrase biasing end to end on the tiny models: ``Engine.ctc_beam_bias`` (through ctc_beam_decode) against
cn_ctc_bias_beam_host and tests/ctc_bias_model.py run on the engine's own captured log-posteriors and their pruned lists (fp32 and
bf16x3), a phrase of the second-best hypothesis that a large enough score makes the best one, ctc_att on the biased beams, and
decode_asr --hip_bias for CassNATTask (ctc_only, ctc_att) and ArtTask (ctc_only) with its refusals; without the flag nothing changes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_bias_cases as cases
import ctc_bias_model as model
from conftest import ast_tiny_case, tiny_case
from cassnat_asr_public_amd.models.bias import BiasList
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode
from test_gpu_ctc_ngram import PIECES40, VOCAB
from test_gpu_ctcbeam import build

pytestmark = pytest.mark.gpu

CONF = dict(ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0)


def nat(prec="fp32", decode_type="ctc_only"):
    args, state, feats, sizes = tiny_case(decode_type=decode_type, sample_num=1, **CONF)
    assert args.vocab_size == 40
    m = build(args, state, prec, capture=True)
    src = torch.from_numpy(feats).cuda()
    return m, args, (src, (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(sizes).cuda())


def ast(prec="fp32"):
    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.models.transformer import make_model

    args, state, feats = ast_tiny_case(ctc_weight=0.3)
    args.decode_type, args.ctc_pruning, args.ctc_lp, args.ctc_lm_weight = "ctc_only", CONF["ctc_pruning"], CONF["ctc_lp"], 0
    _, sizes = synth.make_feats(3, 61, 80, lengths=[61, 57, 51], seed=11)
    args.hip_precision, args.hip_capture = prec, True
    m = make_model(args.input_size, args).cuda()
    with torch.no_grad():
        for k, q in m.named_parameters():
            q.copy_(torch.from_numpy(state[k]))
    src = torch.from_numpy(feats).cuda()
    return m, args, (src, (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(np.asarray(sizes, np.float32)).cuda())


def search(m, args, batch, vocab, bias):
    """ctc_beam_decode, and the log-posteriors, pruned lists and frame counts it ran on."""
    with torch.no_grad():
        top = ctc_beam_decode(m, *batch, vocab, args, None, bias=bias)
    ctc = np.asarray(m.engine(*batch[0].shape[:2]).fetch("ctc_out"), np.float32)
    pruned = torch.topk(torch.from_numpy(ctc), args.ctc_pruning, dim=-1)[1].numpy().astype(np.int32)
    return top, SimpleNamespace(logp=np.ascontiguousarray(ctc), top=np.ascontiguousarray(pruned), ratio=batch[2].cpu().numpy().astype(np.float32),
                                W=int(args.ctc_beam), P=int(args.ctc_pruning), lp=float(args.ctc_lp))


def phrases_of(free, low=0):
    """Phrases cut from the LM-free best hypotheses, a near-miss of each and a penalised one; dyadic scores.  ``low``: the smallest id
    a phrase may hold (a list file cannot name sos / eos)."""
    out = {}
    for utt in free:
        h = utt[0]["hyp"]
        for ids, s in ((h[:2], 2.0), (h[2:5], 0.5), (h[1:3] + h[:1], 3.0), (h[5:7], -1.0)):
            if len(ids) >= 2 and min(ids) >= low:
                out.setdefault(tuple(ids), s)
    assert len(out) >= 2
    return out


def assert_same(top, want, tol=1e-8):
    assert len(top) == len(want)
    for b, utt in enumerate(top):
        assert [s["hyp"] for s in utt] == [s["hyp"] for s in want[b]], b
        assert [s["score_lm"] for s in utt] == [s["score_lm"] for s in want[b]], b
        for key in ("score_ctc", "p_blk", "p_nblk"):
            np.testing.assert_allclose([s[key] for s in utt], [s[key] for s in want[b]], rtol=0, atol=tol, err_msg=key)


@pytest.mark.parametrize("which", ["nat", "ast"])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_the_engine_equals_the_host_entry_and_the_model_on_its_own_log_posteriors(prec, which):
    m, args, batch = nat(prec) if which == "nat" else ast(prec)
    free, _ = search(m, args, batch, VOCAB, None)
    assert all(s["score_lm"] == 0.0 for u in free for s in u)
    phrases = phrases_of(free)
    bias = BiasList.from_phrases(phrases)
    top, case = search(m, args, batch, VOCAB, bias)
    Tp = case.logp.shape[1]
    assert_same(top, cases.run_host(case, bias=bias))
    want = model.search(case.logp, case.top, cases.src_sizes(case.ratio, Tp), case.W, case.lp, phrases, blank=args.padding_idx)
    assert_same(top, want)
    for utt in top:
        for s in utt:
            assert s["ys"].dtype == torch.long and s["ys"][0].tolist() == [1] + s["hyp"]
            assert s["score_lm"] == model.rescan(s["hyp"], phrases)
    assert sum(model.events(s["hyp"], phrases)[0] for u in top for s in u) > 0  # phrases were completed


def second_best_phrase(free_utt):
    """Two neighbouring labels of the first hypothesis whose labels differ from the best's, which the best does not hold in a row."""
    best = free_utt[0]["hyp"]
    pairs = set(zip(best, best[1:]))
    for s in free_utt[1:]:
        for pair in zip(s["hyp"], s["hyp"][1:]):
            if s["hyp"] != best and pair not in pairs:
                return pair, s["hyp"]
    return None, None


def test_a_phrase_of_the_second_best_hypothesis_wins_with_a_large_enough_score():
    m, args, batch = nat("fp32")
    free, case = search(m, args, batch, VOCAB, None)
    b, (phrase, second) = next((b, second_best_phrase(u)) for b, u in enumerate(free) if second_best_phrase(u)[0])
    sizes = cases.src_sizes(case.ratio, case.logp.shape[1])
    for score in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0):  # the smallest at which the model's best hypothesis holds the phrase
        want = model.search(case.logp, case.top, sizes, case.W, case.lp, {phrase: score}, blank=args.padding_idx)
        if model.rescan(want[b][0]["hyp"], {phrase: score}) > 0:
            break
    else:
        raise AssertionError("no score makes the phrase win in the model")
    assert want[b][0]["hyp"] != free[b][0]["hyp"]
    args.hip_bias_model = BiasList.from_phrases({phrase: score})  # (the way decode_asr hands the list over)
    top, _ = search(m, args, batch, VOCAB, None)
    assert top[b][0]["hyp"] == want[b][0]["hyp"] and top[b][0]["score_lm"] == model.rescan(top[b][0]["hyp"], {phrase: score}) >= 2 * score
    assert phrase in set(zip(top[b][0]["hyp"], top[b][0]["hyp"][1:])) and second is not None
    assert_same(top, want)
    # with the flag absent the result is today's
    args.hip_bias_model = None
    again, _ = search(m, args, batch, VOCAB, None)
    assert [[(s["hyp"], s["score_ctc"], s["score_lm"]) for s in u] for u in again] == [[(s["hyp"], s["score_ctc"], s["score_lm"]) for s in u] for u in free]


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_ctc_att_aligns_the_decoder_to_the_biased_best_hypothesis(prec):
    m, args, batch = nat(prec, "ctc_att")
    free, _ = search(m, args, batch, VOCAB, None)
    bias = BiasList.from_phrases(phrases_of(free))
    top, _ = search(m, args, batch, VOCAB, bias)
    with torch.no_grad():
        out, _ = m.beam_decode(*batch, VOCAB, args, None, top)
        forced, _ = m.beam_decode(*batch, VOCAB, args, None, [[{"hyp": list(u[0]["hyp"]), "ys": u[0]["ys"].clone()}] for u in top])
    for a, b in zip(out, forced):
        assert a[0]["hyp"] == b[0]["hyp"] and a[0]["score"] == b[0]["score"]


# ---- decode_asr ----------------------------------------------------------------------------------------------------------------------
def run_cli(tmp, cli, tag, flags=()):
    from cassnat_asr_public_amd.bin import decode_asr

    result = str(tmp / ("result_%s.txt" % tag))
    assert decode_asr.main(cli + ["--result_file", result] + list(flags)) == 0
    return open(result, "rb").read()


def write_list(tmp, phrases, vocab):
    path = tmp / "bias.txt"
    path.write_text("# cut from the best hypotheses\n\n" + "".join("%s\t%r\n" % (" ".join(vocab.index2word[i] for i in ids), s)
                                                                   for ids, s in phrases.items()), encoding="utf-8")
    return str(path)


def lines_of(recog, vocab, args):
    from cassnat_asr_public_amd.tasks.cassnat_task import hyp_to_words

    return ["spk-utt%02d " % b + " ".join(hyp_to_words(seqs[0]["hyp"], vocab, args.padding_idx)) for b, seqs in enumerate(recog)]


@pytest.mark.parametrize("decode_type", ["ctc_only", "ctc_att"])
def test_decode_asr_cassnat_with_a_list(tmp_path, decode_type):
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.data.vocab import Vocab

    m, args, batch = nat("fp32", decode_type)
    vocab_file = tmp_path / "pieces.txt"
    vocab_file.write_text("".join(p + "\n" for p in PIECES40[4:]), encoding="utf-8")
    vocab = Vocab(str(vocab_file), rank=1)
    conf = dict(decode_type=decode_type, sample_num=1, vocab_file=str(vocab_file), **CONF)
    scp, ckpt, cfg = _write_case(tmp_path, args, dict((k, v.detach().cpu().numpy()) for k, v in m.named_parameters()), batch[0].cpu().numpy(),
                                 [61, 50, 37], extra_conf=conf)
    cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "3", "--hip_precision", "fp32",
           "--load_data_workers", "0"]
    free, case = search(m, args, batch, vocab, None)
    phrases = phrases_of(free, low=4)
    flags = ["--hip_bias", write_list(tmp_path, phrases, vocab), "--hip_bias_score", "0.5"]
    # the model's hypotheses on the engine's log-posteriors; with ctc_att the decoder is aligned to the best of them
    want = model.search(case.logp, case.top, cases.src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, phrases, blank=args.padding_idx)
    recog = [[{"hyp": list(s["hyp"]), "ys": torch.tensor([[1] + s["hyp"]], dtype=torch.long)} for s in u] for u in want]
    plain = free
    if decode_type == "ctc_att":
        with torch.no_grad():
            recog, _ = m.beam_decode(*batch, vocab, args, None, recog)
            plain, _ = m.beam_decode(*batch, vocab, args, None, free)
    got = run_cli(tmp_path, cli, "bias", flags)
    assert got.decode("utf-8").splitlines() == lines_of(recog, vocab, args)
    # without the flag: what the LM-free search gives, twice the same bytes
    first = run_cli(tmp_path, cli, "plain")
    assert first.decode("utf-8").splitlines() == lines_of(plain, vocab, args) and run_cli(tmp_path, cli, "plain2") == first
    if decode_type == "ctc_only":
        assert got != first


def test_decode_asr_art_ctc_only_with_a_list(tmp_path):
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.data.vocab import Vocab

    m, args, batch = ast("fp32")
    lengths = [61, 57, 51]
    conf = dict(decode_type="ctc_only", ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0)
    scp, ckpt, cfg = _write_case(tmp_path, args, dict((k, v.detach().cpu().numpy()) for k, v in m.named_parameters()), batch[0].cpu().numpy(),
                                 lengths, extra_conf=conf, ast=True)
    vocab = Vocab(str(tmp_path / "vocab.txt"), rank=1)
    cli = ["--task", "art", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "3", "--hip_precision", "fp32",
           "--load_data_workers", "0"]
    free, case = search(m, args, batch, vocab, None)
    phrases = phrases_of(free, low=4)
    want = model.search(case.logp, case.top, cases.src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, phrases, blank=args.padding_idx)
    got = run_cli(tmp_path, cli, "bias", ["--hip_bias", write_list(tmp_path, phrases, vocab)])
    assert got.decode("utf-8").splitlines() == lines_of(want, vocab, args)
    first = run_cli(tmp_path, cli, "plain")
    assert first.decode("utf-8").splitlines() == lines_of(free, vocab, args) and run_cli(tmp_path, cli, "plain2") == first
    assert got != first


def test_decode_asr_art_workers_share_one_list(tmp_path, monkeypatch):
    """Six batches of one utterance on four decode workers, which all read the one BiasList of the process: its tables are placed
    on the device once, before the workers start, and the result is the single worker's."""
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.data.vocab import Vocab

    m, args, batch = ast("fp32")
    feats = batch[0].cpu().numpy()
    conf = dict(decode_type="ctc_only", ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0)
    scp, ckpt, cfg = _write_case(tmp_path, args, dict((k, v.detach().cpu().numpy()) for k, v in m.named_parameters()),
                                 np.concatenate([feats, feats]), [61, 57, 51] * 2, extra_conf=conf, ast=True)
    vocab = Vocab(str(tmp_path / "vocab.txt"), rank=1)
    free, case = search(m, args, batch, vocab, None)
    phrases = phrases_of(free, low=4)
    want = model.search(case.logp, case.top, cases.src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, phrases, blank=args.padding_idx)
    placed = []
    real = BiasList.cuda
    monkeypatch.setattr(BiasList, "cuda", lambda self, device=None: (placed.append((id(self), len(self._dev))), real(self, device))[1])
    cli = ["--task", "art", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "1", "--hip_precision", "fp32",
           "--load_data_workers", "0", "--hip_bias", write_list(tmp_path, phrases, vocab)]
    four = run_cli(tmp_path, cli, "four", ["--hip_pipelines", "4"])
    assert placed and placed[0][1] == 0 and all(n == 1 for _, n in placed[1:]) and len({i for i, _ in placed}) == 1
    assert four == run_cli(tmp_path, cli, "one", ["--hip_pipelines", "1"])
    lines = four.decode("utf-8").splitlines()
    assert len(lines) == 6 and lines[0].split()[1:] == lines[3].split()[1:] == lines_of(want, vocab, args)[0].split()[1:]  # (the unpadded one)
    assert [ln.split()[1:] for ln in lines[:3]] == [ln.split()[1:] for ln in lines[3:]]


def test_threads_get_one_descriptor_over_tables_placed_once():
    import threading

    bias = BiasList.from_phrases(cases.SETS["probe_wrap"][0])
    dev = torch.device("cuda", torch.cuda.current_device())
    got, gate = [], threading.Barrier(8)

    def worker():
        gate.wait()
        bias.cuda(dev)
        got.append((bias.desc(dev), {k: v.data_ptr() for k, v in bias._dev[dev].items()}))

    threads = [threading.Thread(target=worker) for _ in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(got) == 8 and all(d is got[0][0] and ptrs == got[0][1] for d, ptrs in got)
    assert all(getattr(got[0][0], k) == p for k, p in got[0][1].items())  # the descriptor points at the tables that are kept


def test_decode_asr_refuses_the_flag_where_it_would_be_ignored(tmp_path):
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.data.vocab import Vocab
    from ctc_ngram_model import dyadic_arpa
    from test_gpu_ngram import WORDS

    m, args, batch = nat("fp32")
    vocab_file = tmp_path / "pieces.txt"
    vocab_file.write_text("".join(p + "\n" for p in PIECES40[4:]), encoding="utf-8")
    vocab = Vocab(str(vocab_file), rank=1)
    state = dict((k, v.detach().cpu().numpy()) for k, v in m.named_parameters())
    listfile = write_list(tmp_path, {cases.ids("▁a bc"): 2.0}, vocab)
    arpa = tmp_path / "model.arpa"
    arpa.write_text(dyadic_arpa(WORDS, 3, seed=3), encoding="utf-8")
    runs = ((dict(decode_type="ctc_only", ctc_lm_weight=0.3), ["--rank_model", "n-gram", "--rnnlm", str(arpa)], "ctc_lm_weight"),
            (dict(decode_type="att_only", ctc_lm_weight=0), [], "att_only"),
            (dict(decode_type="att_only", ctc_lm_weight=0, sample_num=4), [], "ESA"))
    for i, (over, more, names) in enumerate(runs):
        sub = tmp_path / ("run%d" % i)
        sub.mkdir()
        conf = dict(dict(sample_num=1, vocab_file=str(vocab_file), **CONF), **over)
        scp, ckpt, cfg = _write_case(sub, args, state, batch[0].cpu().numpy(), [61, 50, 37], extra_conf=conf)
        cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "3", "--hip_precision",
               "fp32", "--load_data_workers", "0", "--result_file", str(sub / "result.txt"), "--hip_bias", listfile] + more
        with pytest.raises(NotImplementedError, match="hip_bias") as e:
            decode_asr.main(cli)
        assert names in str(e.value)
    # a list the loader refuses: the line is named
    bad = tmp_path / "bad.txt"
    bad.write_text("▁a bc\n▁a qq\n", encoding="utf-8")
    with pytest.raises(ValueError, match="line 2"):
        decode_asr.main(cli[:-1] + [str(bad)])
