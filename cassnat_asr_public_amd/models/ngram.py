"""ARPA n-gram language model for the ESA ranker (``rank_model: n-gram``; the reference hands every sample's text to kenlm,
src/models/cassnat.py:522-535).  ``NgramLM.load`` reads the ARPA text into hash tables (csrc/ngram.hip reads it; no package outside
numpy / torch), ``score_tokens`` scores rows of word-piece ids on the device, ``score_tokens_host`` is the same code on the host, and
``score(text)`` has kenlm's signature (``bos=True, eos=True``), so the object also fits the host loop of ``CassNAT._esa_decode``.

Semantics are the documented ARPA ones (include/cassnat_hip.h); kenlm is not a dependency and binary kenlm files are not read.
"""
import ctypes as C
import re
import warnings

import numpy as np
import torch

from .. import hip

SEPARATOR = "▁".encode()  # what the reference replaces by a blank before kenlm splits the text
_ASCII_SPACE = b" \t\n\r\x0b\x0c"
_SPLIT = re.compile(b"[ \t\n\r\x0b\x0c]+")


def _slots(entries):
    """Power of two, at least 2 * (entries + 1): tables stay at most half full."""
    n = 2
    while n < 2 * (entries + 1):
        n *= 2
    return n


def _ptr(a):
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _hash(strings):
    """(H, P^len) of byte strings, by the library (cn_ngram_hash)."""
    off = np.zeros(len(strings) + 1, np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    buf = np.frombuffer(b"".join(strings) + b"\0", np.uint8)
    h, pw = np.zeros(len(strings), np.uint64), np.zeros(len(strings), np.uint64)
    hip.check(hip.lib().cn_ngram_hash(_ptr(buf), _ptr(off), len(strings), _ptr(h), _ptr(pw)), "cn_ngram_hash")
    return h, pw


def split_piece(piece):
    """A vocabulary piece as (begins with a separator, body bytes, the body is free of separators)."""
    b = piece.encode()
    i = 0
    while i < len(b):
        if b.startswith(SEPARATOR, i):
            i += len(SEPARATOR)
        elif b[i] in _ASCII_SPACE:
            i += 1
        else:
            break
    body = b[i:]
    return i > 0, body, SEPARATOR not in body and not any(c in _ASCII_SPACE for c in body)


class NgramLM(object):
    """Tables of one ARPA model and of one vocabulary's pieces.  ``order``, ``n_words``, ``entries``, ``unclosed`` (entries whose
    prefix or suffix is not in the file: there kenlm's incremental matching may differ from the longest-match rule used here),
    ``has_unk``, ``device_ok`` (False: some piece has a separator behind its leading run, only ``score(text)`` is right then)."""

    _TABLES = ("word_keys", "word_ids", "gram_keys", "gram_prob", "gram_bo", "piece_hash", "piece_pow", "piece_starts")
    _warned = False

    @classmethod
    def load(cls, arpa_path, vocab, hash_bits=64):
        L = hip.lib()
        text = np.fromfile(arpa_path, dtype=np.uint8)
        if text.size == 0:
            raise ValueError("%s: empty file" % arpa_path)
        counts = np.zeros(9, np.int64)
        if L.cn_ngram_counts(_ptr(text), text.size, _ptr(counts)) != 0:
            raise ValueError("%s: %s" % (arpa_path, L.cn_last_error().decode(errors="replace")))
        order = int(counts[0])
        ws, gs = _slots(int(counts[1])), _slots(int(counts[1 : order + 1].sum()))
        self = cls()
        t = dict(word_keys=np.zeros(ws, np.uint64), word_ids=np.zeros(ws, np.int32), gram_keys=np.zeros(gs, np.uint64),
                 gram_prob=np.zeros(gs, np.float32), gram_bo=np.zeros(gs, np.float32))
        info = np.zeros(8, np.int64)
        rc = L.cn_ngram_parse(_ptr(text), text.size, int(hash_bits), _ptr(t["word_keys"]), _ptr(t["word_ids"]), ws, _ptr(t["gram_keys"]),
                              _ptr(t["gram_prob"]), _ptr(t["gram_bo"]), gs, _ptr(info))
        if rc != 0:
            raise ValueError("%s: %s" % (arpa_path, L.cn_last_error().decode(errors="replace")))
        self.path, self.hash_bits = arpa_path, int(hash_bits)
        self.order, self.n_words, self.entries, self.unclosed = (int(v) for v in info[:4])
        self.bos, self.eos, self.unk, self.has_unk = int(info[4]), int(info[5]), int(info[6]), bool(info[7])
        self.key_mask = (1 << self.hash_bits) - 1
        if self.unclosed and not NgramLM._warned:
            NgramLM._warned = True
            warnings.warn("%s: %d n-grams lack their prefix or suffix in the file; the longest-match rule used here and kenlm's "
                          "incremental matching can differ on such a model" % (arpa_path, self.unclosed))
        # the vocabulary's pieces
        n = int(getattr(vocab, "n_words", 0)) or len(vocab.index2word)
        parts = [split_piece(vocab.index2word[i]) for i in range(n)]
        self.device_ok = all(ok for _, _, ok in parts)
        t["piece_hash"], t["piece_pow"] = _hash([body for _, body, _ in parts])
        t["piece_starts"] = np.array([s for s, _, _ in parts], np.uint8)
        self.vocab_size = n
        # (torch has no arithmetic on uint64: the keys travel as the same bits in int64)
        self._host = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in t.items()}
        self._dev, self._desc = {}, {}
        self.device = None
        return self

    # ------------------------------------------------------------------------------------------------------------------
    def cuda(self, device=None):
        """Place the tables on a device (kept beside the host copy, which the host scorer reads)."""
        index = device.index if isinstance(device, torch.device) else device
        dev = torch.device("cuda", torch.cuda.current_device() if index is None else int(index))
        if dev not in self._dev:
            self._dev[dev] = {k: v.to(dev) for k, v in self._host.items()}
        self.device = dev
        return self

    def _make_desc(self, tables, vocab=None):
        d = hip.CnNgramDesc()
        for k in self._TABLES:
            setattr(d, k, tables[k].data_ptr())
        d.word_slots, d.gram_slots = tables["word_keys"].numel(), tables["gram_keys"].numel()
        d.vocab = self.vocab_size if vocab is None else vocab
        d.order, d.bos, d.eos, d.unk, d.key_mask = self.order, self.bos, self.eos, self.unk, self.key_mask
        return d

    def desc(self, where="host"):
        """The cn_ngram_desc over the host tables, or over those of a device ``cuda`` placed."""
        if where not in self._desc:
            self._desc[where] = self._make_desc(self._host if where == "host" else self._dev[where])
        return self._desc[where]

    def _need_pieces(self):
        if not self.device_ok:
            raise ValueError("a piece of the vocabulary has a separator behind its leading run: token rows cannot be scored, use score(text)")

    # ------------------------------------------------------------------------------------------------------------------
    def score(self, text, bos=True, eos=True):
        """log10 P(words </s> | <s>) of a text split at ASCII white space - ``kenlm.Model.score(text)`` with its defaults."""
        if not (bos and eos):
            raise NotImplementedError("NgramLM.score: bos=True, eos=True only")
        words = [w for w in _SPLIT.split(text.encode() if isinstance(text, str) else bytes(text)) if w]
        if not words:
            words = [b""]  # (one empty piece: no word, the sentence is </s> alone)
        h, pw = _hash(words)
        tables = dict(self._host, piece_hash=torch.from_numpy(h.view(np.int64)), piece_pow=torch.from_numpy(pw.view(np.int64)),
                      piece_starts=torch.ones(len(words), dtype=torch.uint8))
        d = self._make_desc(tables, vocab=len(words))
        tok, n, out = np.arange(len(words), dtype=np.int32), np.array([len(words)], np.int32), np.zeros(1, np.float32)
        hip.check(hip.lib().cn_ngram_score_host(C.byref(d), _ptr(tok), len(words), _ptr(n), 1, -1, _ptr(out)), "cn_ngram_score_host")
        return float(out[0])

    def score_tokens_host(self, tok, ylen, drop_id=2):
        """tok int32 (rows, stride), ylen int32 (rows,), numpy -> float32 (rows,): every row's first ylen ids, those equal to
        ``drop_id`` left out, glued into words as the reference's text path does and scored as ``score`` would."""
        self._need_pieces()
        tok, ylen = np.ascontiguousarray(tok, np.int32), np.ascontiguousarray(ylen, np.int32)
        rows, stride = tok.shape
        assert ylen.shape == (rows,)
        out = np.zeros(rows, np.float32)
        hip.check(hip.lib().cn_ngram_score_host(C.byref(self.desc()), _ptr(tok), stride, _ptr(ylen), rows, int(drop_id), _ptr(out)),
                  "cn_ngram_score_host")
        return out

    def ast_adds_host(self, rows, lens, eos):
        """rows int32 (n, ld), lens int32 (n,), numpy -> float32 (n, 2): per hypothesis (tokens behind sos) what a token that begins
        a word and what eos add in the AST beam search (include/cassnat_hip_ast_ngram.h), on the host."""
        self._need_pieces()
        rows, lens = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(lens, np.int32)
        n, ld = rows.shape
        assert lens.shape == (n,)
        out = np.zeros((n, 2), np.float32)
        hip.check(hip.lib().cn_ast_ngram_adds_host(C.byref(self.desc()), _ptr(rows), ld, _ptr(lens), n, int(eos), _ptr(out)),
                  "cn_ast_ngram_adds_host")
        return out

    def score_tokens(self, tok, ylen, drop_id=2):
        """The same on the device: CUDA int32 tensors (rows, stride) and (rows,) -> CUDA float32 (rows,), on the current stream."""
        self._need_pieces()
        assert tok.is_cuda and tok.dtype == torch.int32 and ylen.dtype == torch.int32 and tok.dim() == 2 and ylen.numel() == tok.shape[0]
        dev = tok.device
        if dev not in self._dev:
            self.cuda(dev)
        tok, ylen = tok.contiguous(), ylen.to(dev).contiguous()
        out = torch.zeros(tok.shape[0], dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            hip.check(hip.lib().cn_op_ngram_score(C.byref(self.desc(dev)), _ptr(tok), tok.shape[1], _ptr(ylen), tok.shape[0], int(drop_id),
                                                  _ptr(out), hip.current_stream()), "cn_op_ngram_score")
        return out
