"""Scoring a run against its references (``decode_asr --hip_score DIR``, ``bin/score_asr``): the word / token / character error rate
from the device's weighted edit alignment (``hip.edit_align``; include/cassnat_hip_score.h).  This module is the host side: reading the
two files, turning lines into units and ids, one device call over all pairs of the run, and the files.  Not in the reference, whose
recipes end in text2trn.py, spm_decode and sclite.  A post-pass over strings: no decode path knows of it.

Files.  The hypothesis file is a result file (``UTT piece piece ...``).  The reference file (``--hip_score_ref``, default
``--text_label``) has one line per utterance, ``UTT unit unit ...``, in pieces (``--hip_score_ref_form pieces``, what token.scp holds) or
in words; its text is read as it stands, not the loader's unk-mapped ids.

Units (``--hip_score_unit``).  ``word``: pieces merge at the separator, by ``utils.ctm.units``, so the words are the CTM's words; for a
vocabulary without separator pieces it falls back to ``token`` (the rule of ``ctm.unit_of``).  ``token``: the pieces themselves; refused
with a reference in words.  ``char``: the characters of the words.

Alignment.  Costs ``--hip_score_costs S,I,D`` (default 1,1,1, Kaldi's compute-wer; sclite's weights are 4,3,3); on equal cost the
first of (diagonal, deletion, insertion) wins at every cell, seen from the end of the pair.  Under 1,1,1 the total is the edit distance
and independent of the tie rule; the split into S / D / I follows the rule and may differ from sclite's.  No text normalisation.

Modes.  ``present``: an utterance of the reference file with no hypothesis is skipped and counted as not present; ``all``: its
reference counts as deletions.  An utterance of the hypothesis file without a reference is an error."""
import os

import numpy as np

from . import ctm

MAX_UNITS = 8192            # the op's bound on a side of a pair
SCRATCH_BOUND = 1 << 30     # bytes of back-pointers one device call may ask for
UNITS = ("word", "token", "char")
STAR = "***"


class ScoreError(ValueError):
    pass


def parse_costs(text):
    """``S,I,D`` -> (sub, ins, del), each in 1 .. 255."""
    try:
        costs = tuple(int(x) for x in str(text).split(","))
    except ValueError:
        costs = ()
    if len(costs) != 3 or any(c < 1 or c > 255 for c in costs):
        raise ScoreError("hip_score_costs: expected S,I,D with each cost in 1 .. 255, got %r" % (text,))
    return costs


def read_table(path):
    """``UTT field field ...`` lines -> (utterances in file order, utt -> fields); a repeated utterance is an error."""
    order, table = [], {}
    with open(path, encoding="utf-8") as f:
        for raw in f:
            fields = raw.split()
            if not fields:
                continue
            if fields[0] in table:
                raise ScoreError("%s: utterance %s appears twice" % (path, fields[0]))
            order.append(fields[0])
            table[fields[0]] = fields[1:]
    return order, table


def unit_of(unit, vocab):
    """``word`` becomes ``token`` for a vocabulary without separator pieces (``ctm.unit_of``'s rule); ``vocab`` None: as asked."""
    if unit not in UNITS:
        raise ScoreError("hip_score_unit: %r is none of %s" % (unit, ", ".join(UNITS)))
    return "token" if unit == "word" and vocab is not None and not ctm.has_separator(vocab) else unit


def to_units(fields, form, unit):
    """The units of one line: ``form`` pieces or words, ``unit`` word, token or char."""
    if unit == "token":
        if form != "pieces":
            raise ScoreError("hip_score_unit token needs a reference in pieces (--hip_score_ref_form pieces)")
        return list(fields)
    words = [text for _, _, text in ctm.units(list(fields), "word")] if form == "pieces" else list(fields)
    return words if unit == "word" else [ch for w in words for ch in w]


def _align(ref_units, hyp_units, costs, host, flavour):
    """Ids from one dictionary over both sides, every pair to the aligner in one call (more only to bound its scratch) -> per pair
    (counts [C, S, D, I], path codes)."""
    from .. import hip

    ids = {}
    for side in (ref_units, hyp_units):
        for us in side:
            for u in us:
                ids.setdefault(u, len(ids))
    out = []
    N = len(ref_units)
    at = 0
    while at < N:
        # (a call's launch is sized by its longest pair: the back-pointers of n pairs take n * max_ref * ceil((max_hyp + 1) / 64) * 16 bytes)
        n, mr, mh = 0, 0, 0
        while at + n < N:
            r, h = max(mr, len(ref_units[at + n])), max(mh, len(hyp_units[at + n]))
            if n and (n + 1) * r * ((h + 64) // 64) * 16 > SCRATCH_BOUND:
                break
            n, mr, mh = n + 1, r, h
        refs, hyps = ref_units[at:at + n], hyp_units[at:at + n]
        ref = np.fromiter((ids[u] for us in refs for u in us), np.int32)
        hyp = np.fromiter((ids[u] for us in hyps for u in us), np.int32)
        rl, hl = np.array([len(us) for us in refs], np.int32), np.array([len(us) for us in hyps], np.int32)
        rb, hb = np.cumsum(rl, dtype=np.int64) - rl, np.cumsum(hl, dtype=np.int64) - hl
        if host:
            _, counts, plen, ops, ob = hip.edit_align_host(ref, rb, rl, hyp, hb, hl, costs, mr, mh, flavour=flavour)
        else:
            import torch

            dev = torch.device("cuda", torch.cuda.current_device())
            got = hip.edit_align(*(torch.from_numpy(a).to(dev) for a in (ref, rb, rl, hyp, hb, hl)), costs=costs, max_ref=mr, max_hyp=mh,
                                 flavour=flavour)
            _, counts, plen, ops, ob = (t.cpu().numpy() for t in got)
        for k in range(n):
            out.append((counts[k].tolist(), ops[ob[k]:ob[k] + plen[k]].tolist()))
        at += n
    return out


class Result:
    """``utts``: the scored utterances in order; per utterance ``ref`` / ``hyp`` units, ``counts`` [C, S, D, I], ``path`` codes."""

    def __init__(self, unit, costs, utts, ref, hyp, counts, path, not_present):
        self.unit, self.costs, self.utts, self.ref, self.hyp, self.counts, self.path, self.not_present = unit, costs, utts, ref, hyp, counts, path, not_present

    def totals(self):
        c, s, d, i = (sum(self.counts[u][k] for u in self.utts) for k in range(4))
        return c, s, d, i

    def wer_lines(self):
        c, s, d, i = self.totals()
        n_ref, errs = c + s + d, s + d + i
        wrong = sum(1 for u in self.utts if sum(self.counts[u][1:]))
        return ["%%WER %.2f [ %d / %d, %d ins, %d del, %d sub ]" % (100.0 * errs / n_ref, errs, n_ref, i, d, s),
                "%%SER %.2f [ %d / %d ]" % (100.0 * wrong / len(self.utts), wrong, len(self.utts)),
                "Scored %d sentences, %d not present in hyp." % (len(self.utts), self.not_present),
                "unit %s, costs sub %d ins %d del %d" % ((self.unit,) + tuple(self.costs))]

    def per_utt_lines(self, utt):
        ref, hyp = iter(self.ref[utt]), iter(self.hyp[utt])
        r_col, h_col = [], []
        for op in self.path[utt]:
            r_col.append(next(ref) if op != 3 else STAR)
            h_col.append(next(hyp) if op != 2 else STAR)
        c, s, d, i = self.counts[utt]
        return [" ".join([utt, "ref"] + r_col), " ".join([utt, "hyp"] + h_col), " ".join([utt, "op"] + ["CSDI"[op] for op in self.path[utt]]),
                "%s #csid %d %d %d %d" % (utt, c, s, i, d)]

    def write(self, out_dir):
        os.makedirs(out_dir, exist_ok=True)

        def put(name, lines):
            with open(os.path.join(out_dir, name), "w", encoding="utf-8") as f:
                for line in lines:
                    print(line, file=f)

        put("wer", self.wer_lines())
        put("per_utt", [line for u in self.utts for line in self.per_utt_lines(u)])
        put("ref.trn", [" ".join(self.ref[u] + ["(%s)" % u]) for u in self.utts])
        put("hyp.trn", [" ".join(self.hyp[u] + ["(%s)" % u]) for u in self.utts])


def score(order, hyps, ref_order, refs, unit="word", ref_form="pieces", costs=(1, 1, 1), mode="present", host=False, flavour=None):
    """``order`` / ``hyps``: the hypothesis utterances in output order and their pieces; ``ref_order`` / ``refs``: the reference file's.
    ``unit`` is final here (``unit_of`` has been applied).  -> ``Result``."""
    if mode not in ("present", "all"):
        raise ScoreError("hip_score_mode: %r is neither present nor all" % (mode,))
    if ref_form not in ("pieces", "words"):
        raise ScoreError("hip_score_ref_form: %r is neither pieces nor words" % (ref_form,))
    for utt in order:
        if utt not in refs:
            raise ScoreError("utterance %s of the hypothesis file has no reference" % utt)
    absent = [utt for utt in ref_order if utt not in hyps]
    utts = list(order) + (absent if mode == "all" else [])
    ref_units = {utt: to_units(refs[utt], ref_form, unit) for utt in utts}
    hyp_units = {utt: to_units(hyps.get(utt, []), "pieces", unit) for utt in utts}
    for utt in utts:
        if max(len(ref_units[utt]), len(hyp_units[utt])) > MAX_UNITS:
            raise ScoreError("utterance %s has more than %d units" % (utt, MAX_UNITS))
    if not any(ref_units[utt] for utt in utts):
        raise ScoreError("the references of the scored utterances hold no unit at all")
    got = _align([ref_units[u] for u in utts], [hyp_units[u] for u in utts], costs, host, flavour)
    return Result(unit, costs, utts, ref_units, hyp_units, {u: g[0] for u, g in zip(utts, got)}, {u: g[1] for u, g in zip(utts, got)}, len(absent))


def score_files(hyp_file, ref_file, out_dir, vocab=None, unit="word", ref_form="pieces", costs=(1, 1, 1), mode="present", host=False, order=None,
                hyps=None):
    """Score ``hyp_file`` (or the given ``order`` / ``hyps``) against ``ref_file``, write the four files into ``out_dir``, print and
    return the %WER line."""
    if hyps is None:
        order, hyps = read_table(hyp_file)
    ref_order, refs = read_table(ref_file)
    res = score(order, hyps, ref_order, refs, unit_of(unit, vocab), ref_form, costs, mode, host)
    res.write(out_dir)
    line = res.wer_lines()[0]
    print(line, flush=True)
    return line


def score_run(args, vocab, order, hyps, host=False):
    """The post-pass of a decode task on rank 0: ``hyps`` utt -> the pieces just written to the result file, ``order`` the scp's."""
    ref_file = getattr(args, "hip_score_ref", "") or getattr(args, "text_label", "")
    if not ref_file:
        raise ScoreError("--hip_score needs references: --hip_score_ref FILE or --text_label FILE")
    return score_files(None, ref_file, args.hip_score, vocab, getattr(args, "hip_score_unit", "word") or "word",
                       getattr(args, "hip_score_ref_form", "pieces") or "pieces", parse_costs(getattr(args, "hip_score_costs", "1,1,1") or "1,1,1"),
                       getattr(args, "hip_score_mode", "present") or "present", host, order, hyps)
