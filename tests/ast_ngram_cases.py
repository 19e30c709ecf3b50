"""Inputs shared by tests/test_ast_ngram_host.py and the GPU tests of the AST beam search with word n-gram fusion: the crafted token
rows, random rows, the host entry as a function and the model's adds for a batch of rows."""
import ctypes as C

import numpy as np

import ast_ngram_model as model_of
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import _ptr
from ctc_ngram_cases import ORDERS, VOCAB, IX, V, WORDS, lm_of  # noqa: F401  (re-exported)

EOS, SOS, BLANK = IX["eos"], IX["sos"], IX["blank"]
NEW = ["cn_ast_attach_ngram", "cn_op_ast_ngram_adds", "cn_ast_ngram_adds_host", "cn_op_ast_ngram_terms", "cn_op_logsoftmax_class_topk",
       "cn_ast_step_ngram"]
SENT = -7.5


def crafted(ld):
    """The rows every adds test walks: (list of id lists, each at most ld long; the row of full length ld is among them)."""
    rng = np.random.RandomState(3)
    w = lambda *names: [IX[n] for n in names]  # noqa: E731
    pieces = [i for i in range(V) if i != EOS]
    rows = [
        [],                                                             # empty
        w("▁a", "bc"),                                                  # an open word only
        w("a", "b"),                                                    # ... without a separator in front
        w("▁ab", "▁"),                                                  # ending in a bare separator
        w("▁"),
        w("▁▁a"), w("▁c", "▁▁a", "b"), w("▁", "▁", "▁a"),               # doubled separators
        w("▁zz", "a"), w("▁a", "▁zz", "a", "▁b"), w("▁zz", "▁zz", "▁"),  # words outside the model
        w("▁a", "▁b", "▁c", "▁ab", "▁ba", "▁cc", "▁aa", "▁bb", "▁ca", "▁a", "bc"),  # more than 7 closed words, one open
        w("▁a", "▁b", "▁c", "▁ab", "▁ba", "▁cc", "▁aa", "▁bb", "▁ca", "▁"),         # ... none open
        w("▁a", "eos", "bc", "eos", "▁c"), w("eos"), w("▁ab", "c", "eos"),          # eos ids inside the row
        [int(t) for t in rng.choice(pieces, ld)],                                   # a row of full length
        w("▁a") + [-3] + w("bc") + [V, 1000] + w("▁c"), [-1], [V + 5, -(2 ** 31), 2 ** 31 - 1],  # ids outside [0, V)
        w("blank", "sos", "unk", "▁a", "sos"),                                     # the specials are pieces like any other
    ]
    assert all(len(r) <= ld for r in rows) and any(len(r) == ld for r in rows)
    return rows


def random_rows(rng, n, ld, p_start=0.45):
    """n rows of random length in [0, ld]: word-starting and continuation pieces, now and then eos or a foreign id."""
    starts = [i for i in range(V) if VOCAB.index2word[i].startswith("▁")]
    conts = [i for i in range(V) if not VOCAB.index2word[i].startswith("▁") and i != EOS]
    rows = []
    for _ in range(n):
        row = []
        for _ in range(rng.randint(0, ld + 1)):
            u = rng.rand()
            row.append(EOS if u < 0.03 else (int(rng.randint(-5, V + 5)) if u < 0.06 else
                                             int(rng.choice(starts if rng.rand() < p_start else conts))))
        rows.append(row)
    return rows


def pack(rows, ld, fill=EOS + 1000):
    """(tok (n, ld) int32 with garbage behind every row's length, len (n,) int32)."""
    tok = np.full((len(rows), ld), fill, np.int32)
    for r, row in enumerate(rows):
        tok[r, :len(row)] = row
    return tok, np.array([len(r) for r in rows], np.int32)


def host_adds(lm, tok, lens, eos=EOS, pad=8):
    """cn_ast_ngram_adds_host on packed rows; the output has ``pad`` more floats than the entry may write, which must stay."""
    n, ld = tok.shape
    out = np.full(2 * n + pad, SENT, np.float32)
    rc = hip.lib().cn_ast_ngram_adds_host(C.byref(lm.desc()), _ptr(tok), ld, _ptr(lens), n, eos, _ptr(out))
    assert rc == 0, hip.lib().cn_last_error()
    assert (out[2 * n:] == SENT).all()
    return out[:2 * n].reshape(n, 2)


def model_adds(model, rows, eos=EOS):
    return np.array([model_of.adds(model, VOCAB, r, eos) for r in rows], np.float32).reshape(len(rows), 2)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    bad = np.argwhere(a.view(np.int32) != b.view(np.int32))
    assert bad.size == 0, (bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])
