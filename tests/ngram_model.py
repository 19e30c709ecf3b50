"""float64, dict-based restatement of the n-gram ranker's semantics (the issue's "What the numbers must mean"; no kenlm here):

  * the text of a token row is built as the reference does (src/models/cassnat.py:522-531): drop every token equal to 2, concatenate
    ``vocab.index2word[t]``, replace U+2581 by a blank, strip, split at white space;
  * score = log10 P(w_1 .. w_m </s> | <s>) with textbook ARPA back-off: the history is the last c = min(order - 1, words so far + 1)
    words starting with <s>; p is the probability of the longest k-gram (k = c + 1 .. 1) in the model; then the back-off weights of
    the j-grams of the last j history words are added for j = k .. c; an absent n-gram or weight adds nothing; a word the model does
    not know is <unk>, whose probability is -100 when the file has no <unk>.

``score`` returns (score, sum |terms|, number of terms): a float32 sum of m terms taken in order is within m * 2^-24 * sum |terms|
of it (first order: every term rounded to float32 once and m - 1 rounded additions).
"""
import re
from collections import Counter

import numpy as np

_WS = re.compile("[ \t\n\r\x0b\x0c]+")
UNK_MISSING = -100.0


class ArpaModel(object):
    def __init__(self, text):
        self.grams, self.order = {}, 0
        k = 0
        for line in text.split("\n"):
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\"):
                k = int(line[1 : line.index("-")])
                self.order = max(self.order, k)
                continue
            f = line.split()
            assert len(f) in (k + 1, k + 2), line
            self.grams[tuple(f[1 : k + 1])] = (float(f[0]), float(f[k + 1]) if len(f) == k + 2 else None)
        self.hits = Counter()  # order of the n-gram that gave a word's probability -> count

    def words_of(self, text):
        return [w for w in _WS.split(text) if w]

    def score(self, text):
        hist, terms = ["<s>"], []
        for w in self.words_of(text) + ["</s>"]:
            if (w,) not in self.grams:
                w = "<unk>"
            c = min(self.order - 1, len(hist))
            ctx = hist[len(hist) - c :]
            k, p = 1, UNK_MISSING
            for kk in range(c + 1, 0, -1):
                g = tuple(ctx[c - (kk - 1) :]) + (w,)
                if g in self.grams:
                    k, p = kk, self.grams[g][0]
                    break
            self.hits[k] += 1
            terms.append(p)
            for j in range(k, c + 1):
                g = tuple(ctx[c - j :])
                if g in self.grams and self.grams[g][1] is not None:
                    terms.append(self.grams[g][1])
            hist.append(w)
        total = 0.0
        for t in terms:
            total += t
        return total, float(sum(abs(t) for t in terms)), len(terms)

    def bound(self, text):
        _, mass, m = self.score(text)
        return m * 2.0 ** -24 * mass


def text_of(row, n, vocab, drop_id=2):
    """The reference's text of a token row (cassnat.py:527-531)."""
    return "".join(vocab.index2word[int(t)] for t in row[:n] if int(t) != drop_id).replace("▁", " ").strip()


def score_tokens(model, tok, ylen, vocab, drop_id=2):
    """Per row: (score, sum |terms|, terms)."""
    return [model.score(text_of(row, int(n), vocab, drop_id)) for row, n in zip(tok, ylen)]


def random_arpa(words, order, seed, unk=True, sep="\t", keep=0.5, bo_skip=0.3):
    """A random CLOSED ARPA text over ``words``: orders 1 .. order, every n-gram's prefix and suffix (n - 1)-gram in the file, <s> only
    in front, </s> only at the end; no back-off column on the highest order, behind </s>, and on a share ``bo_skip`` of the rest."""
    rng = np.random.RandomState(seed)
    uni = (["<unk>"] if unk else []) + ["<s>", "</s>"] + list(words)
    levels = [[(w,) for w in uni]]
    for n in range(2, order + 1):
        prev, have, nxt = levels[-1], set(levels[-1]), []
        for g in prev:
            if g[-1] == "</s>":
                continue
            for w in uni:
                if w == "<s>" or g[1:] + (w,) not in have:
                    continue
                if rng.rand() < keep:
                    nxt.append(g + (w,))
        levels.append(nxt)
    while levels and not levels[-1]:
        levels.pop()
    out = ["\\data\\"] + ["ngram %d=%d" % (n + 1, len(g)) for n, g in enumerate(levels)] + [""]
    for n, grams in enumerate(levels):
        out.append("\\%d-grams:" % (n + 1))
        for g in grams:
            p = "-99" if g == ("<s>",) else "%.4f" % -rng.uniform(0.05, 3.0)
            fields = [p, " ".join(g)]
            if n + 1 < len(levels) and g[-1] != "</s>" and (g == ("<s>",) or rng.rand() >= bo_skip):
                fields.append("%.4f" % -rng.uniform(0.0, 1.5))
            out.append(sep.join(fields))
        out.append("")
    out.append("\\end\\")
    return "\n".join(out) + "\n"
