"""CTM output (``decode_asr --hip_ctm FILE``): word time stamps and confidences from the device's forced CTC alignment of the best
hypothesis (``hip.Engine.ctc_token_times``; include/cassnat_hip_ctc_times.h).  This module is the host side: aligning a batch's
hypotheses, turning token spans into units and writing the file.  Not in the reference.

Units.  The hypothesis' pieces become words: a word starts at the first piece and at every piece that begins with the separator
(``models.ngram.SEPARATOR``); a vocabulary in which no piece begins with it - and ``--hip_ctm_unit token`` - is written per token.  A
word starts where its first piece starts, ends where its last piece ends, and its confidence is exp of the smallest ``conf_lp`` of its
pieces (``conf_lp``: the largest CTC log-posterior of the piece inside its span).

Timing.  One subsampled frame is ``4 * skip_frame * frame_shift`` seconds (two stride-2 convolutions behind the frame skipping), the
frame shift that of ``--hip_fbank_conf`` when given, else 10 ms.  A span of frames [s, e) is written as start ``s`` and duration ``e - s``
of those units: no receptive-field offset is applied, although a subsampled frame sees input frames on both sides of the four it stands for.

Line.  ``UTT 1 START DUR WORD CONF`` with ``%.2f %.2f ... %.3f``; with ``--hip_segments`` ``REC 1 (segment start + START) DUR WORD CONF``,
the segment start being first / rate of its sample range (``data.segments``).  An empty hypothesis writes no line.  An utterance the aligner could
not align (status not 0, a label the walk never entered, a path of probability zero) spreads its units evenly over its valid frames
with confidence 0.000."""
import math

import numpy as np
import torch

from ..models.ngram import SEPARATOR

SEP = SEPARATOR.decode()
DEFAULT_FRAME_SHIFT = 0.010


def frame_shift_of(args):
    """Seconds per input frame: ``--hip_fbank_conf``'s frame shift when the flag is given, else 10 ms."""
    if getattr(args, "hip_fbank_conf", "") or "":
        from ..data.speech_loader import front_end_options

        return float(front_end_options(args).frame_shift_ms) * 0.001
    return DEFAULT_FRAME_SHIFT


def seconds_per_frame(args):
    """Seconds per subsampled frame: 4 * skip_frame * frame shift."""
    return 4 * int(getattr(args, "skip_frame", 1) or 1) * frame_shift_of(args)


def has_separator(vocab):
    """Does any piece of the vocabulary begin with the separator?"""
    return any(str(w).startswith(SEP) for w in vocab.index2word.values())


def unit_of(args, vocab):
    """"word" or "token": ``--hip_ctm_unit`` (default word), and token for a vocabulary without separator pieces."""
    unit = getattr(args, "hip_ctm_unit", "word") or "word"
    return unit if unit == "token" or has_separator(vocab) else "token"


def label_ids(hyp, vocab, padding_idx):
    """The ids ``tasks.cassnat_task.hyp_to_words`` turns into the result line: no sos, no padding (= the blank), up to the first eos."""
    sos, eos = vocab.word2index["sos"], vocab.word2index["eos"]
    out = []
    for idx in hyp:
        idx = int(idx)
        if idx == sos or idx == padding_idx:
            continue
        if idx == eos:
            break
        out.append(idx)
    return out


def align_batch(model, src, src_size, args, hyps, vocab, engine=None):
    """Forced alignment of one batch's best hypotheses (``hyps``: token lists as the decoders return them) on the model's engine - or
    on ``engine``, a decode worker's own: -> per utterance the record ``lines`` reads, ``(pieces, start, end, conf_lp, status,
    n_frames)`` of plain Python values (it travels between ranks).  Encodes the batch again."""
    from .. import hip

    ids = [label_ids(h, vocab, args.padding_idx) for h in hyps]
    B, ld = len(ids), max(1, max((len(y) for y in ids), default=0))
    labels = np.zeros((B, ld), np.int32)
    for b, y in enumerate(ids):
        labels[b, :len(y)] = y
    dev = torch.device("cuda", getattr(model, "_device", torch.cuda.current_device()))
    feats = src.to(dev, torch.float32).contiguous()
    ratio = src_size.to(dev, torch.float32).contiguous()
    eng = engine if engine is not None else model.engine(B, feats.shape[1])
    opts = hip.Engine.make_opts(args, capture=getattr(args, "hip_capture", False))
    opts.sos = vocab.word2index["sos"]
    lab = torch.from_numpy(labels).to(dev)
    llen = torch.tensor([len(y) for y in ids], dtype=torch.int32, device=dev)
    start, end, conf, _, status = eng.ctc_token_times(feats, ratio, opts, lab, llen)
    start, end, conf, status = (t.cpu().numpy() for t in (start, end, conf, status))
    frames = valid_frames(feats, args.padding_idx)
    return [([vocab.index2word[i] for i in y], start[b, :len(y)].tolist(), end[b, :len(y)].tolist(), conf[b, :len(y)].tolist(), int(status[b]),
             int(frames[b])) for b, y in enumerate(ids)]


def valid_frames(feats, padding_idx):
    """Valid subsampled frames per utterance, as the engine's key mask counts them: frame j is valid when
    ``feats[b, 4 j, 0] != padding_idx`` (the mask behind the two stride-2 convolutions); padding makes the valid frames a prefix."""
    from ..hip import subsampled

    return (feats[:, ::4, 0][:, :subsampled(feats.shape[1])] != padding_idx).sum(1).cpu().numpy()


def units(pieces, unit):
    """Index ranges [first, last] of the pieces of every unit, and the unit's text (a word: its pieces joined, separators removed)."""
    if unit == "token":
        return [(i, i, p) for i, p in enumerate(pieces)]
    out = []
    for i, p in enumerate(pieces):
        if i == 0 or p.startswith(SEP):
            out.append([i, i, ""])
        out[-1][1] = i
        out[-1][2] += p
    # (a unit of separators alone is no word: the detokenised line has none there either)
    return [(a, b, text.replace(SEP, "")) for a, b, text in out if text.replace(SEP, "")]


def aligned(record):
    pieces, start, end, conf, status, _ = record
    return status == 0 and all(s >= 0 and e > s for s, e in zip(start, end))


def lines(utt, record, sec, unit, offset=None):
    """The CTM lines of one utterance.  ``offset``: (recording, seconds) of an utterance that is a segment of a recording
    (``--hip_segments``) - the lines then carry the recording's id and times in the recording."""
    if offset is not None:
        return ["%s 1 %.2f %.2f %s %.3f" % (offset[0], offset[1] + s, d, text, c) for s, d, text, c in _rows(record, sec, unit)]
    return ["%s 1 %.2f %.2f %s %.3f" % (utt, s, d, text, c) for s, d, text, c in _rows(record, sec, unit)]


def _rows(record, sec, unit):
    """(start, duration, text, confidence) of every unit of one utterance, times in seconds from the utterance's start."""
    pieces, start, end, conf, status, n = record
    us = units(pieces, unit)
    out = []
    if not aligned(record):  # the units share the utterance's frames evenly, confidence 0
        for k, (_, _, text) in enumerate(us):
            s, e = n * k / len(us), n * (k + 1) / len(us)
            out.append((s * sec, (e - s) * sec, text, 0.0))
        return out
    for a, b, text in us:
        c = math.exp(min(conf[a:b + 1]))
        out.append((start[a] * sec, (end[b] - start[a]) * sec, text, min(1.0, max(0.0, c))))
    return out


def write(path, order, records, sec, unit, offsets=None):
    """Writes the file in the utterance order ``order``; returns the number of utterances that were not aligned (empty hypotheses
    do not count).  ``offsets``: {utt: (recording, segment start in seconds)} under ``--hip_segments`` (``lines``)."""
    unaligned = 0
    with open(path, "w", encoding="utf-8") as f:
        for utt in order:
            rec = records[utt]
            if rec[0] and not aligned(rec):
                unaligned += 1
            for line in lines(utt, rec, sec, unit, None if offsets is None else offsets[utt]):
                print(line, file=f)
    return unaligned
