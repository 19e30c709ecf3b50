"""Kaldi `segments` files on the audio path (``--hip_segments``): an utterance is a sample range of a recording.  Pure Python.

One segment per line, `UTT REC START END`, times in seconds; END = -1 means the end of the recording.  REC names a line of the
wav.scp.  A recording may carry any number of segments, overlapping or not; the segments are the utterances, in the file's order; a
recording without segments is not decoded.  A fifth field (Kaldi's channel) is refused: the channel comes from `--channel` of the
front end's option file.

The sample range, at the file's own rate and before any resampling (as `extract-segments | compute-fbank-feats` would cut it):

    first = floor(START * rate + 0.5)        last = floor(END * rate + 0.5)

Kaldi TRUNCATES (first = int(START * rate)) where this rounds: a time printed with three decimals then names the sample it was
computed from (``bin/make_segments`` prints such times); the two differ by at most one sample.  ``last`` beyond the file by up to
0.5 s is cut to the file.  Everything else that Kaldi skips with a warning is an error here, raised before anything is decoded and
naming segment and recording - a decode that silently loses utterances is worse: ``last`` further beyond the file, a negative START,
an empty or inverted segment, an unknown recording, a duplicate id, a segment that gives no analysis frame."""
import math

OVERSHOOT_SECONDS = 0.5


def _who(utt, rec):
    return "segment %s of recording %s" % (utt, rec)


def read_segments(path):
    """-> [(utt, rec, start, end)] in the file's order (blank lines are skipped)."""
    out, seen = [], set()
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            fields = raw.split()
            if not fields:
                continue
            if len(fields) == 5:
                raise ValueError("segments %s line %d: segment %s carries a fifth field (%s): a channel per segment is not read, the "
                                 "channel comes from --channel of --hip_fbank_conf" % (path, no, fields[0], fields[4]))
            if len(fields) != 4:
                raise ValueError("segments %s line %d: not `UTT REC START END`: %r" % (path, no, raw.rstrip("\n")))
            utt, rec = fields[0], fields[1]
            try:
                start, end = float(fields[2]), float(fields[3])
            except ValueError:
                raise ValueError("segments %s line %d: %s: START and END must be numbers (got %s %s)" % (path, no, _who(utt, rec), fields[2], fields[3]))
            if not (math.isfinite(start) and math.isfinite(end)):
                raise ValueError("segments %s line %d: %s: START and END must be finite" % (path, no, _who(utt, rec)))
            if utt in seen:
                raise ValueError("segments %s line %d: %s: the id is a duplicate" % (path, no, _who(utt, rec)))
            seen.add(utt)
            out.append((utt, rec, start, end))
    if not out:
        raise ValueError("segments %s: no segment" % path)
    return out


def sample_of(seconds, rate):
    """floor(seconds * rate + 0.5)"""
    return int(math.floor(float(seconds) * int(rate) + 0.5))


def sample_range(start, end, rate, samples, utt="?", rec="?"):
    """The range [first, last) of a recording of ``samples`` samples per channel at ``rate`` Hz; raises as the module says."""
    if start < 0:
        raise ValueError("%s: START = %s is negative" % (_who(utt, rec), start))
    first = sample_of(start, rate)
    last = int(samples) if end == -1 else sample_of(end, rate)
    if last > samples:
        if last - samples > OVERSHOOT_SECONDS * rate:
            raise ValueError("%s: END = %s lies %.3f s beyond the recording's %d samples at %d Hz (up to %.1f s is cut to the file)"
                             % (_who(utt, rec), end, (last - samples) / rate, samples, rate, OVERSHOOT_SECONDS))
        last = int(samples)
    if last <= first:
        raise ValueError("%s: START = %s, END = %s: the segment is empty or inverted (samples [%d, %d) of %d)"
                         % (_who(utt, rec), start, end, first, last, samples))
    return first, last


def check_recordings(segs, recordings, path=""):
    """Every REC names a line of the wav.scp."""
    known = set(recordings)
    for utt, rec, _, _ in segs:
        if rec not in known:
            raise ValueError("segments %s: %s: the recording is unknown (no such line in the wav.scp)" % (path, _who(utt, rec)))


def rough_frames(args):
    """Per segment of ``--hip_segments`` its duration in units of 10 ms: what orders the utterance list by length (sharding,
    --hip_bucket) before the dataset has read a header.  A segment that ends with its recording takes the length from the file."""
    from . import kaldi_io, wave_io

    table, lengths, out = dict(kaldi_io.read_scp(args.test_paths[0]["scp_path"])), {}, []
    for utt, rec, start, end in read_segments(args.hip_segments):
        if end == -1 and rec in table:
            if rec not in lengths:
                rate, channels, _, _, _, nbytes = wave_io.read_header(table[rec], rec)
                lengths[rec] = nbytes / max(1, 2 * channels * rate)
            end = lengths[rec]
        out.append(max(0, int(round((end - start) * 100))))
    return out


def utterance_order(args):
    """The ids of a decode run's utterances in output order: the segments' with ``--hip_segments``, else the first fields of the scp."""
    path = getattr(args, "hip_segments", "") or ""
    if path:
        return [utt for utt, _, _, _ in read_segments(path)]
    return [line.split()[0] for line in open(args.test_paths[0]["scp_path"]) if line.strip()]
