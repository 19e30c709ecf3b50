"""Contextual phrase biasing ("hot words") for the CTC prefix beam search (``--hip_bias FILE``; include/cassnat_hip_ctc_bias.h holds
the semantics; csrc/ctc_bias_search.h walks the tables) and, with ``--hip_bias_search att``, for the AST beam search
(include/cassnat_hip_ast_bias.h; csrc/ast_bias_search.h).  ``BiasList.load`` reads a phrase list written in vocabulary pieces into an
Aho-Corasick automaton, ``cuda(dev)`` places its tables on a device and ``desc(dev)`` gives the ``cn_bias_desc`` over them - the manner
of models.ngram.NgramLM.  The automaton is built on the host in plain Python and numpy (the tables travel as torch tensors, the
descriptor is hip.CnBiasDesc); no tokenizer is involved.

One ``BiasList`` serves all decode workers of a process: ``cuda`` and ``desc`` take a lock, a device's tables are placed once and
never replaced, so a descriptor handed out stays valid as long as the object lives.
"""
import ctypes as C
import math
import threading

import numpy as np
import torch

from .. import hip

MAX_PIECES = 32
_M32 = 0xFFFFFFFF


def edge_hash(node, piece):
    """cb_hash of csrc/ctc_bias_search.h: where the probing of (node, piece) starts, before the masks."""
    h = ((node * 0x9E3779B1) & _M32) ^ ((piece * 0x85EBCA6B) & _M32)
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & _M32
    h ^= h >> 12
    return h


def _slots(entries):
    """Power of two, at least 4 * (entries + 1): the table stays at most a quarter full (most look-ups miss, and a miss walks to the
    end of its probe run)."""
    n = 2
    while n < 4 * (entries + 1):
        n *= 2
    return n


def value_ok(pieces, score):
    """float32(pieces) * float32(score), the value of a phrase's last node, is finite (a finite score near the float32 limit is not)."""
    with np.errstate(over="ignore"):
        return bool(np.isfinite(np.float32(pieces) * np.float32(score)))


def read_phrases(path, vocab, score=3.0):
    """The phrase list as {tuple of piece ids: per-piece score}; a refusal names the file and the line."""
    if not math.isfinite(float(score)):
        raise ValueError("hip_bias_score must be finite, not %r" % (score,))
    banned = {vocab.word2index[w] for w in ("blank", "sos", "eos") if w in vocab.word2index}
    phrases = {}
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            where = "%s: line %d" % (path, no)
            s = float(score)
            if "\t" in line:
                line, _, tail = line.rpartition("\t")
                try:
                    s = float(tail)
                except ValueError:
                    raise ValueError("%s: the score %r is no number" % (where, tail))
                if not math.isfinite(s):
                    raise ValueError("%s: the score %r is not finite" % (where, tail))
            pieces = line.split()
            if not pieces:
                raise ValueError("%s: a score without a phrase" % where)
            if len(pieces) > MAX_PIECES:
                raise ValueError("%s: a phrase of %d pieces (at most %d)" % (where, len(pieces), MAX_PIECES))
            ids = []
            for p in pieces:
                if p not in vocab.word2index:
                    raise ValueError("%s: the piece %r is not in the vocabulary" % (where, p))
                if vocab.word2index[p] in banned:
                    raise ValueError("%s: %r cannot be part of a phrase" % (where, p))
                ids.append(int(vocab.word2index[p]))
            if not value_ok(len(ids), s):
                raise ValueError("%s: %d pieces times the score %r is not finite in float32" % (where, len(ids), s))
            ids = tuple(ids)
            phrases[ids] = max(phrases.get(ids, -math.inf), s)
    return phrases


class BiasList(object):
    """The automaton of one phrase list.  ``phrases`` {ids: score}, ``nodes``, ``edges``, ``slots``, ``hash_bits``; host arrays
    ``child`` (list of dicts), ``depth``, ``fail``, ``hit``, ``value``, ``bank``, ``reset``, ``edge_keys``, ``edge_child``."""

    _TABLES = ("edge_keys", "edge_child", "fail", "value", "bank", "reset")

    @classmethod
    def load(cls, path, vocab, score=3.0, hash_bits=32):
        self = cls.from_phrases(read_phrases(path, vocab, score), hash_bits=hash_bits)
        self.path = path
        return self

    @classmethod
    def from_phrases(cls, phrases, hash_bits=32):
        """``phrases``: {tuple of piece ids: per-piece score} (or pairs; a duplicate keeps the larger score)."""
        if not 0 <= int(hash_bits) <= 32:
            raise ValueError("hash_bits must lie in 0 .. 32")
        merged = {}
        for ids, s in (phrases.items() if isinstance(phrases, dict) else phrases):
            ids = tuple(int(i) for i in ids)
            if not ids or len(ids) > MAX_PIECES or min(ids) < 0 or not math.isfinite(float(s)) or not value_ok(len(ids), s):
                raise ValueError("a phrase needs 1 .. %d piece ids and a score whose product with their count is finite in float32: %r"
                                 % (MAX_PIECES, (ids, s)))
            merged[ids] = max(merged.get(ids, -math.inf), float(s))
        self = cls()
        self.path, self.phrases, self.hash_bits = None, merged, int(hash_bits)
        # the trie: node 0 the root; best[n] the largest score of the phrases through n
        child, depth, best, ends = [{}], [0], [-math.inf], [False]
        for ids, s in merged.items():
            n = 0
            for c in ids:
                if c not in child[n]:
                    child[n][c] = len(child)
                    child.append({})
                    depth.append(depth[n] + 1)
                    best.append(-math.inf)
                    ends.append(False)
                n = child[n][c]
                best[n] = max(best[n], s)
            ends[n] = True
        N = len(child)
        # failure links and hits, breadth first (a node's failure target is shallower: already done)
        fail, hit = [0] * N, [-1] * N
        queue = list(child[0].values())
        for n in queue:
            hit[n] = n if ends[n] else -1
        at = 0
        while at < len(queue):
            n = queue[at]
            at += 1
            for c, m in child[n].items():
                f = fail[n]
                while f and c not in child[f]:
                    f = fail[f]
                fail[m] = child[f][c] if c in child[f] and child[f][c] != m else 0
                hit[m] = m if ends[m] else hit[fail[m]]
                queue.append(m)
        value = np.zeros(N, np.float32)
        for n in range(1, N):
            value[n] = np.float32(depth[n]) * np.float32(best[n])
        bank = np.array([value[h] if h >= 0 else 0.0 for h in hit], np.float32)
        reset = np.array([h >= 0 for h in hit], np.uint8)
        # the edges, hashed: linear probing downwards from the masked hash
        edges = [(n, c, m) for n in range(N) for c, m in child[n].items()]
        slots = _slots(len(edges))
        keys, kids = np.full(slots, -1, np.int64), np.zeros(slots, np.int32)
        mask = ((1 << self.hash_bits) - 1) & (slots - 1)
        for n, c, m in edges:
            i = edge_hash(n, c) & mask
            while keys[i] >= 0:
                i = (i - 1) & (slots - 1)
            keys[i], kids[i] = (n << 32) | c, m
        self.nodes, self.edges, self.slots = N, len(edges), slots
        self.child, self.depth, self.hit = child, depth, hit
        self.fail, self.value, self.bank, self.reset = np.array(fail, np.int32), value, bank, reset
        self.edge_keys, self.edge_child = keys, kids
        self._host = {k: torch.from_numpy(getattr(self, k)) for k in self._TABLES}
        self._dev, self._desc = {}, {}
        self._lock = threading.Lock()
        self.device = None
        return self

    def cuda(self, device=None):
        """Place the tables on a device (kept beside the host copy, which the host search reads)."""
        index = device.index if isinstance(device, torch.device) else device
        dev = torch.device("cuda", torch.cuda.current_device() if index is None else int(index))
        with self._lock:  # (decode workers share the object: the first places the tables, nobody replaces them)
            if dev not in self._dev:
                self._dev[dev] = {k: v.to(dev) for k, v in self._host.items()}
            self.device = dev
        return self

    def desc(self, where="host"):
        """The cn_bias_desc over the host tables, or over those of a device ``cuda`` placed."""
        with self._lock:
            return self._desc_locked(where)

    # ---- the AST beam search's share (include/cassnat_hip_ast_bias.h), on the host: what Transformer.beam_decode's hip_host_beam loop asks
    def ast_nodes_host(self, rows, lens):
        """The node of every hypothesis ``rows`` int32 (n, ld), row r its first ``lens[r]`` ids WITHOUT sos -> int32 (n,)
        (cn_ast_bias_nodes_host: the device's step function on the host tables)."""
        rows = np.ascontiguousarray(rows, np.int32)
        rows = rows.reshape(len(rows), -1)
        lens = np.ascontiguousarray(lens, np.int32).reshape(-1)
        assert lens.size == rows.shape[0]
        out = np.zeros(rows.shape[0], np.int32)
        if rows.shape[0] == 0:
            return out
        if rows.shape[1] == 0:  # (the entry wants a stride; rows without a column are empty hypotheses)
            rows, lens = np.zeros((rows.shape[0], 1), np.int32), np.zeros_like(lens)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        L = hip.lib()
        hip.check(L.cn_ast_bias_nodes_host(C.byref(self.desc()), p(rows), rows.shape[1], p(lens), rows.shape[0], p(out)),
                  "cn_ast_bias_nodes_host", L)
        return out

    def ast_terms_host(self, nodes, idx, eos):
        """The terms float32 (n, K) of the candidates ``idx`` int32 (n, K) for hypotheses at ``nodes`` int32 (n,)
        (cn_ast_bias_terms_host)."""
        nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        idx = np.ascontiguousarray(idx, np.int32)
        idx = idx.reshape(nodes.size, -1)
        out = np.zeros(idx.shape, np.float32)
        if idx.size == 0:
            return out
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        L = hip.lib()
        hip.check(L.cn_ast_bias_terms_host(C.byref(self.desc()), p(nodes), int(eos), p(idx), idx.shape[0], idx.shape[1], p(out)),
                  "cn_ast_bias_terms_host", L)
        return out

    def _desc_locked(self, where):
        if where not in self._desc:
            tables = self._host if where == "host" else self._dev[where]
            d = hip.CnBiasDesc()
            for k in self._TABLES:
                setattr(d, k, tables[k].data_ptr())
            d.slots, d.nodes, d.hash_bits, d.reserved = self.slots, self.nodes, self.hash_bits, 0
            self._desc[where] = d
        return self._desc[where]
