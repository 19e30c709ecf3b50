"""numpy float32 restatement of what a word n-gram model adds in the AST beam search (include/cassnat_hip_ast_ngram.h).  Nothing here
comes from the code under test: the text of a hypothesis is ctc_ngram_model.raw_of's, its words closed_and_open's, the scores
WordModel.word_score's (the float32 sum of the ARPA terms in their order).

adds(hyp) = (a_word, a_eos): a_word is the score of the open word after the closed ones (0 when none is open), a_eos that plus the
score of </s> behind it, added in float32.  term(c) is a_eos for eos, a_word for a piece that begins with a separator, else 0.
Ids outside the vocabulary contribute no piece, like eos.
"""
import numpy as np

from ctc_ngram_model import closed_and_open, raw_of

F32 = np.float32


def pieces_of(hyp, vocab):
    """The ids of ``hyp`` (no sos) that name a piece."""
    n = len(vocab.index2word)
    return [int(t) for t in hyp if 0 <= int(t) < n]


def adds(model, vocab, hyp, eos):
    closed, opened = closed_and_open(raw_of(pieces_of(hyp, vocab), vocab, drop_id=eos))
    hist = ["<s>"] + [model.known(w) for w in closed]
    if opened is None:
        return np.array([0.0, model.word_score(hist, "</s>")], F32)
    w = model.known(opened)
    close32, end32 = F32(model.word_score(hist, w)), F32(model.word_score(hist + [w], "</s>"))
    return np.array([close32, F32(close32 + end32)], F32)


def starts_of(vocab):
    """uint8 per piece: it begins with a separator."""
    return np.array([vocab.index2word[i].startswith("▁") for i in range(len(vocab.index2word))], np.uint8)


def term(a, starts, eos, c):
    """The term of candidate token ``c`` for a hypothesis with adds ``a``."""
    c = int(c)
    if c == eos:
        return F32(a[1])
    return F32(a[0]) if 0 <= c < len(starts) and starts[c] else F32(0.0)


def terms(a, starts, eos, idx):
    """adds (n, 2), candidates (n, K) -> float32 (n, K)."""
    return np.array([[term(a[r], starts, eos, c) for c in idx[r]] for r in range(len(idx))], F32).reshape(np.shape(idx))


def closed_words(model, vocab, hyp, eos):
    return closed_and_open(raw_of(pieces_of(hyp, vocab), vocab, drop_id=eos))[0]
