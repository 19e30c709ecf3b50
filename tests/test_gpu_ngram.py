"""The ARPA n-gram ranker on the device: cn_op_ngram_score (csrc/ngram.hip, one wave per row) bit-equal to cn_ngram_score_host, the
same scoring core on the host; ESA decoding ranked by an NgramLM on the device against the same decode through the host loop; and
decode_asr with `rank_model: n-gram` and an ARPA file in --rnnlm."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import tiny_case
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import NgramLM
from ngram_model import ArpaModel, random_arpa, text_of

pytestmark = pytest.mark.gpu

SPECIALS = ["blank", "sos", "eos", "unk"]
WORDS = ["ab", "ba", "abc", "abcbc", "c", "cc", "bca", "a", "b", "cab", "bb", "ac", "ca", "aa", "bcb", "cbc"]  # the 16-word model
CONT = ["a", "b", "c", "bc", "cb"]
PIECES = SPECIALS + ["▁" + w for w in WORDS] + CONT + ["▁", "▁▁a", "▁zz"]
VOCAB = SimpleNamespace(index2word=dict(enumerate(PIECES)), n_words=len(PIECES))
IX = {p: i for i, p in enumerate(PIECES)}
SENTINEL = 7.0


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """order -> (NgramLM on the device, the float64 model of the same text)"""
    out = {}
    d = tmp_path_factory.mktemp("ngram_gpu")
    for order in (1, 2, 3, 5):
        text = random_arpa(WORDS, order, seed=order, unk=order != 2, keep=0.5 if order < 5 else 0.35)
        path = d / ("o%d.arpa" % order)
        path.write_text(text, encoding="utf-8")
        lm = NgramLM.load(str(path), VOCAB).cuda()
        assert lm.order == order and lm.device_ok and lm.unclosed == 0
        out[order] = (lm, ArpaModel(text))
    return out


def spell(words):
    """One piece per word."""
    return [IX["▁" + w] for w in words]


def both(lm, tok, ylen, drop_id=2):
    """(device scores, host scores); the device buffer has 8 more floats than rows, which must stay untouched."""
    rows = tok.shape[0]
    host = lm.score_tokens_host(tok, ylen, drop_id)
    out = torch.full((rows + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    t, n = torch.from_numpy(tok).cuda(), torch.from_numpy(ylen).cuda()
    rc = hip.lib().cn_op_ngram_score(C.byref(lm.desc(lm.device)), hip._ptr(t), tok.shape[1], hip._ptr(n), rows, drop_id, hip._ptr(out),
                                     hip.current_stream())
    assert rc == 0, hip.lib().cn_last_error()
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[rows:] == SENTINEL).all()
    return out[:rows], host


def same_bits(a, b):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_device_scores_are_the_host_scores_bit_for_bit(models, order):
    lm, model = models[order]
    rng = np.random.RandomState(100 + order)
    top = sorted(g for g in model.grams if len(g) == order and "<s>" not in g and "</s>" not in g and "<unk>" not in g)
    model.hits.clear()
    for rows, stride in ((1, 1), (5, 63), (5, 64), (5, 65), (3, 130)):
        tok = rng.randint(0, len(PIECES), (rows, stride)).astype(np.int32)
        ylen = rng.randint(0, stride + 1, rows).astype(np.int32)
        ylen[0] = stride
        if rows > 1:
            ylen[-1] = 0
            walk = sum((spell(top[i]) for i in rng.randint(0, len(top), stride // order + 1)), [])[:stride]  # n-grams of the highest order
            tok[1, : len(walk)] = walk
            ylen[1] = len(walk)
        dev, host = both(lm, tok, ylen)
        same_bits(dev, host)
        for row, n in zip(tok, ylen):
            model.score(text_of(row, int(n), VOCAB))
        if rows == 1:
            dev, host = both(lm, tok, np.zeros(1, np.int32))
            same_bits(dev, host)
            assert abs(float(dev[0]) - model.score("")[0]) < 1e-5
    assert all(model.hits[k] > 0 for k in range(1, order + 1)), model.hits  # every order gave some word's probability


def test_crafted_rows(models):
    lm, model = models[3]
    stride = 130
    rng = np.random.RandomState(5)
    one_piece = spell([WORDS[i] for i in rng.randint(0, 16, stride)])
    rows = []
    # a word whose pieces sit at 62 .. 66 ("abcbc", in the model), one-piece words around it
    rows.append(one_piece[:62] + [IX["▁a"], IX["b"], IX["c"], IX["b"], IX["c"]] + one_piece[67:])
    rows.append(one_piece)                                   # 130 one-piece words: the history crosses two chunk boundaries
    rows.append([2] * stride)                                # only dropped tokens
    rows.append([len(PIECES), -1, IX["▁ab"], 1 << 30, IX["c"], -(1 << 31), IX["▁c"]] + one_piece[7:70] + [len(PIECES) + 5] * 60)
    rows.append([IX["a"], IX["b"]] + [2] * 100 + [IX["c"], IX["bc"]] + one_piece[:20] + [IX["▁"]] * 6)  # one word across dropped tokens
    tok = np.array(rows, np.int32)
    ylen = np.array([stride, stride, stride, stride, stride], np.int32)
    dev, host = both(lm, tok, ylen)
    same_bits(dev, host)
    # the float64 model on the rows whose text it can build
    for r in (0, 1, 2, 4):
        ref, mass, m = model.score(text_of(tok[r], stride, VOCAB))
        assert abs(float(dev[r]) - ref) <= m * 2.0 ** -24 * mass, (r, dev[r], ref)
    assert text_of(tok[0], stride, VOCAB).split()[62] == "abcbc" and text_of(tok[4], stride, VOCAB).split()[0] == "abcbc"
    assert abs(float(dev[2]) - model.score("")[0]) < 1e-5
    # another drop id
    dev, host = both(lm, tok, ylen, drop_id=IX["▁ab"])
    same_bits(dev, host)


def test_refusals(models):
    lm, _ = models[3]
    L = hip.lib()
    tok = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    n = torch.full((2,), 4, dtype=torch.int32, device="cuda")
    out = torch.full((4,), SENTINEL, dtype=torch.float32, device="cuda")
    good = lm.desc(lm.device)

    def call(desc=good, tok_p=hip._ptr(tok), stride=4, len_p=hip._ptr(n), rows=2, out_p=hip._ptr(out)):
        rc = L.cn_op_ngram_score(C.byref(desc) if desc is not None else None, tok_p, stride, len_p, rows, 2, out_p, hip.current_stream())
        return rc, L.cn_last_error()

    def edited(**kw):
        d = hip.CnNgramDesc()
        C.memmove(C.byref(d), C.byref(good), C.sizeof(d))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert L.cn_ngram_desc_size() == C.sizeof(hip.CnNgramDesc)
    for kw, msg in ((dict(desc=None), b"null"), (dict(tok_p=None), b"null"), (dict(len_p=None), b"null"), (dict(out_p=None), b"null"),
                    (dict(rows=0), b"positive"), (dict(stride=0), b"positive"), (dict(rows=-1), b"positive"),
                    (dict(desc=edited(order=0)), b"order"), (dict(desc=edited(order=9)), b"order"),
                    (dict(desc=edited(word_slots=good.word_slots - 1)), b"powers of two"), (dict(desc=edited(gram_slots=0)), b"powers of two"),
                    (dict(desc=edited(gram_prob=None)), b"null table"), (dict(desc=edited(piece_pow=None)), b"null table"),
                    (dict(desc=edited(vocab=-1)), b"vocab")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[2:] == SENTINEL).all() and (out.cpu().numpy()[:2] != SENTINEL).all()
    # the host entry refuses the same way
    rc = L.cn_ngram_score_host(C.byref(edited(order=9)), None, 4, None, 2, 2, None)
    assert rc != 0 and b"null" in L.cn_last_error()


# ---- ESA end to end --------------------------------------------------------------------------------------------------------------
ESA_SEED = 3


def esa_lm(tmp_path, vocab):
    words = sorted({w.replace("▁", "") for w in vocab.index2word.values()} - {""})
    path = tmp_path / "esa.arpa"
    path.write_text(random_arpa(words, 3, seed=17, keep=0.3), encoding="utf-8")
    return NgramLM.load(str(path), vocab), str(path)


def test_esa_ranked_on_the_device_is_the_host_loop(tmp_path):
    from test_gpu_ctcbeam import Vocab, build

    args, state, feats, sizes = tiny_case(sample_num=4, threshold=0.9, rank_model="n-gram")
    args.esa_select = np.random.RandomState(ESA_SEED).randint(0, 2, (3 * 4, 16, 1)).astype(np.uint8)
    model = build(args, state, "fp32")
    lm, _ = esa_lm(tmp_path, Vocab)
    lm.cuda()
    seen = []

    class Spy(object):  # the device path, keeping what the ranker returned
        device_ok = True
        score = lm.score

        def score_tokens(self, tok, ylen, drop_id=2):
            out = lm.score_tokens(tok, ylen, drop_id)
            seen.append((out.cpu().numpy(), ylen.cpu().numpy(), tuple(tok.shape)))
            return out

    src = torch.from_numpy(feats).cuda()
    mask, ratio = (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(sizes).cuda()
    host_calls = []

    def host_score(text):
        host_calls.append(text)
        return lm.score(text)

    with torch.no_grad():
        dev_out, _ = model.beam_decode(src, mask, ratio, Vocab, args, Spy())
        direct, _ = model.beam_decode(src, mask, ratio, Vocab, args, lm)
        host_out, _ = model.beam_decode(src, mask, ratio, Vocab, args, SimpleNamespace(score=host_score))  # forces today's host loop
    assert len(seen) == 1 and seen[0][2][0] == 12 and len(host_calls) == 12
    for a, b, c in zip(dev_out, host_out, direct):
        assert a[0]["hyp"] == b[0]["hyp"] == c[0]["hyp"] and a[0]["score"] == b[0]["score"] == c[0]["score"]
    sc, ylen, _ = seen[0]
    np.testing.assert_array_equal(sc.view(np.int32), np.array([lm.score(t) for t in host_calls], np.float32).reshape(3, 4).T.reshape(-1).view(np.int32))
    pick = (sc.astype(np.float64) / ylen).reshape(4, 3).argmax(0)
    assert (pick != 0).any(), pick  # the ranking decides something: some utterance's pick is not the best path


def test_decode_asr_cli_with_an_arpa_file(tmp_path):
    """decode_asr --task cassnat with sample_num 4, rank_model n-gram, ctc_lm_weight 0.1 and --rnnlm model.arpa: no kenlm, and the
    result file is the one the host loop gives through beam_decode on the same draws."""
    import sys

    from test_gpu_ctcbeam import build
    from test_gpu_multirank import _write_case
    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.data.vocab import Vocab
    from cassnat_asr_public_amd.tasks.cassnat_task import hyp_to_words

    args, state, feats, sizes = tiny_case(sample_num=4, threshold=0.9, rank_model="n-gram")
    lengths = [61, 50, 37]
    select = np.random.RandomState(ESA_SEED).randint(0, 2, (3 * 4, 16, 1)).astype(np.uint8)
    scp, ckpt, cfg = _write_case(tmp_path, args, state, feats, lengths,
                                 extra_conf=dict(sample_num=4, threshold=0.9, rank_model="n-gram", ctc_lm_weight=0.1,
                                                 esa_select=select.reshape(-1).tolist()))
    vocab = Vocab(str(tmp_path / "vocab.txt"), rank=1)
    # (this vocabulary's pieces carry no separator, so every sample is one long word, unknown to any model: the samples differ in
    # score / n through n alone - the same numbers on both paths is what is checked)
    words = ["w%d" % i for i in range(8)]
    arpa = tmp_path / "model.arpa"
    arpa.write_text(random_arpa(words, 2, seed=4), encoding="utf-8")
    result = str(tmp_path / "result.txt")
    had = sys.modules.get("kenlm", "absent")
    sys.modules["kenlm"] = None  # an `import kenlm` fails
    try:
        rc = decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                              "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0", "--rnnlm", str(arpa)])
    finally:
        if had == "absent":
            del sys.modules["kenlm"]
        else:
            sys.modules["kenlm"] = had
    assert rc == 0
    lm = NgramLM.load(str(arpa), vocab)
    args.esa_select = select
    model = build(args, state, "fp32")
    src = torch.from_numpy(feats).cuda()
    with torch.no_grad():
        out, _ = model.beam_decode(src, (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(sizes).cuda(), vocab, args,
                                   SimpleNamespace(score=lm.score))
    expect = ["spk-utt%02d " % b + " ".join(hyp_to_words(seqs[0]["hyp"], vocab, args.padding_idx)) for b, seqs in enumerate(out)]
    assert open(result).read().splitlines() == expect
