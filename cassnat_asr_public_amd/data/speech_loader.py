"""Test-time feature pipeline of the reference (src/data/speech_loader.py): Kaldi ark -> global CMVN -> splice /
skip -> zero-padded batch + length ratios.  Only what CassNATTask("test") uses is mirrored (SpeechDataset,
SpeechDataLoader); the training-only DynamicDataset / SSL loaders are out of scope.
"""
import collections
import functools
import os
import threading

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import flac_io, kaldi_io, segments, wave_io
from .feat_op import context_feat, skip_feat


class SingleSet(object):
    """One {name, scp_path[, text_label]} stream -> list of (utt, ark specifier, token ids)."""

    def __init__(self, vocab, data_path, rank=0, segs=None):
        """``segs``: the segments of ``--hip_segments`` ([(utt, rec, start, end)]) - the entries of the scp are then recordings and
        the items the segments of those recordings, in the segments file's order; ``ranges`` keeps their (rec, start, end)."""
        self.name = data_path["name"]
        entries = kaldi_io.read_scp(data_path["scp_path"])
        self.ranges, self.recordings = None, [utt for utt, _ in entries]
        if segs is not None:
            table = dict(entries)
            mine = [g for g in segs if g[1] in table]
            entries, self.ranges = [(utt, table[rec]) for utt, rec, _, _ in mine], [(rec, start, end) for _, rec, start, end in mine]
        if rank == 0:
            print("Reading %d lines from %s" % (len(entries), data_path["scp_path"]))
        labels = None
        if "text_label" in data_path:
            labels = {}
            unk, sos, eos = vocab.word2index["unk"], vocab.word2index["sos"], vocab.word2index["eos"]
            with open(data_path["text_label"], "r") as f:
                for line in f:
                    utt, _, text = line.strip().partition(" ")
                    labels[utt] = [sos] + [vocab.word2index.get(w, unk) for w in text.split(" ")] + [eos]
        self.items = [(utt, spec, labels[utt] if labels is not None else [1]) for utt, spec in entries]

    def get_len(self):
        return len(self.items)


def splice_triple(left, right, skip):
    """(left, right, skip) of a set that splices or skips frames, None for one that does neither (skip 0 and 1 both keep every
    frame: feat_op.skip_feat)."""
    left, right, skip = int(left), int(right), max(1, int(skip))
    return None if (left == 0 and right == 0 and skip == 1) else (left, right, skip)


def spliced_frames(n, splice):
    """Rows the dataset hands out for an utterance of ``n`` source rows: zero rows are appended up to a multiple of ``skip`` before
    every ``skip``-th row is kept (src/data/speech_loader.py:150-156), so n_out = ceil(n / skip); splicing keeps the count."""
    if not splice or splice[2] <= 1:
        return int(n)
    return -(-int(n) // splice[2])


def splice_host(mat, splice, cmvn=None):
    """Steps 1-4 of the dataset's general path on one matrix: the CMVN in float64, rows of literal zeros up to a multiple of skip,
    ``context_feat``, ``skip_feat``.  What collate then rounds to float32 - the definition the device kernel (``hip.splice_rows``)
    is held to."""
    left, right, skip = splice if splice else (0, 0, 1)
    feat = mat if cmvn is None else (mat - cmvn[0]) / cmvn[1]
    rem = feat.shape[0] % skip if skip > 1 else 0
    if rem:
        feat = np.vstack([feat, np.zeros((skip - rem, feat.shape[1]))])
    return skip_feat(context_feat(feat, left, right), skip)


class WaveBatch(object):
    """What a wave set's collate puts where the padded feature tensor would stand: the utterances' int16 sample views and their
    frame counts.  ``shape`` is the padded FEATURE shape (B, longest frame count, num_mel) - with a ``splice`` triple the spliced one,
    (B, longest spliced count, (left + right + 1) * num_mel); ``frames`` stay the front-end's own counts -, so that batch counting,
    progress printing and ``first.shape[1]`` work as for a tensor; the features themselves are computed on the device, in the task's
    own process (``Fbank.packed`` / the packed reader's wave form).  ``formats``: per utterance the file's (rate, channels) - the
    views then hold the interleaved data chunks and ``frames`` count the RESAMPLED wave's frames; None: mono files at the
    front-end's rate.  ``index``: per utterance the ``flac_io.FlacIndex`` of a FLAC set - the views are then the files' uint8 frame
    bytes, decoded on the device, and ``formats`` is always given."""

    __slots__ = ("views", "frames", "utts", "shape", "dtype", "is_cuda", "splice", "formats", "index")

    def __init__(self, views, frames, num_mel, utts=None, splice=None, formats=None, index=None):
        self.views, self.frames, self.utts = list(views), [int(n) for n in frames], utts
        self.index = None if index is None else list(index)
        self.formats = None if formats is None else [(int(r), int(c)) for r, c in formats]
        self.splice = splice_triple(*splice) if splice else None
        blocks = (self.splice[0] + self.splice[1] + 1) if self.splice else 1
        self.shape = (len(self.views), max(spliced_frames(n, self.splice) for n in self.frames), blocks * int(num_mel))
        self.dtype = torch.float32
        self.is_cuda = False


class FlacFrames(object):
    """What a FLAC set hands out per utterance where a wave set hands out samples: ``view`` - a read-only uint8 view of the
    memory-mapped file from its first audio frame to the end - and ``index``, the file's ``flac_io.FlacIndex``."""

    __slots__ = ("view", "index")

    def __init__(self, view, index):
        self.view, self.index = view, index


def front_end(args):
    """The front-end ``--hip_fbank_conf`` describes (default: the built-in options): its option block is ``.o``, ``.admit()`` says
    which files it takes (`--allow-downsample`, `--allow-upsample`, `--channel`)."""
    from .fbank import Fbank

    conf = getattr(args, "hip_fbank_conf", "") or ""
    return Fbank.from_conf(conf) if conf else Fbank()


def front_end_options(args):
    """The fbank option block (``hip.CnFbankOpts``) of ``--hip_fbank_conf`` (default: the built-in options)."""
    return front_end(args).o


def frames_of(opts, samples):
    """Frame count of ``samples`` samples under the option block ``opts`` (snip_edges: cn_fbank_num_frames' rule)."""
    flen, shift = int(opts.sample_rate * 0.001 * opts.frame_length_ms), int(opts.sample_rate * 0.001 * opts.frame_shift_ms)
    return 0 if samples < flen or shift < 1 else 1 + (samples - flen) // shift


def sniff_wave_set(items, mode="auto"):
    """Is the list of (utt, spec, ...) a wave set?  Decided from EVERY entry (``wave_io.entry_kind``): all RIFF/WAVE files - True;
    all FLAC entries (``flac_io.is_flac``) - "flac" (FLAC entries mixed with WAV files or feature matrices raise); none - False (``mode`` "1": an error); a command, a WAV with a `:offset`, or WAV files mixed with anything else raise a
    ValueError that names the utterance.  ``mode`` "0": never look."""
    mode = str(mode)
    if mode == "0":
        return False
    seen = {}  # (entries of one archive share its path: one look per file)

    def kind(spec):
        spec = spec.strip()
        if spec.endswith("|"):
            return "flac" if flac_io.is_flac(spec) else "pipe"
        path, _, off = spec.rpartition(":")
        has_off = bool(path) and off.isdigit()
        name = path if has_off else spec
        if name not in seen:
            seen[name] = "wav" if wave_io.is_wav(name) else ("flac" if not has_off and flac_io.is_flac(name) else None)
        if seen[name] != "wav":
            return seen[name]
        return "wav_offset" if has_off else "wav"

    kinds = [kind(it[1]) for it in items]
    for it, k in zip(items, kinds):
        if k in ("pipe", "wav_offset"):
            wave_io.check_spec(it[1], it[0])
    n_wav = sum(1 for k in kinds if k == "wav")
    n_flac = sum(1 for k in kinds if k == "flac")
    if n_flac:  # a FLAC set: every entry a FLAC stream (a plain path, or the recipe's `flac -c -d -s FILE |`)
        if n_flac != len(items):
            odd, odd_kind = next((it, k) for it, k in zip(items, kinds) if k != "flac")
            raise ValueError("the set mixes FLAC entries and %s: utterance %s (%s) is not a FLAC stream, utterance %s is"
                             % ("WAV files" if odd_kind == "wav" else "feature matrices", odd[0], odd[1],
                                next(it for it, k in zip(items, kinds) if k == "flac")[0]))
        return "flac"
    if n_wav == 0:
        if mode == "1":
            raise ValueError("--hip_audio 1: utterance %s (%s) is not a RIFF/WAVE file" % (items[0][0], items[0][1]) if items
                             else "--hip_audio 1: an empty utterance list")
        return False
    if n_wav != len(items):
        odd = next(it for it, k in zip(items, kinds) if k != "wav")
        raise ValueError("the set mixes WAV files and feature matrices: utterance %s (%s) is not a RIFF/WAVE file, utterance %s is"
                         % (odd[0], odd[1], next(it for it, k in zip(items, kinds) if k == "wav")[0]))
    return True


# --hip_segments keeps one memory map per recording; every map holds a descriptor of its file, so a set of more recordings than this
# keeps the most recently used ones (a map that goes is closed with the last view into it, and mapped again when a segment asks)
MAX_SEGMENT_MAPS = 256


class SpeechDataset(Dataset):
    def __init__(self, vocab, data_paths, args):
        self.left_context, self.right_context = args.left_ctx, args.right_ctx
        self.skip_frame = args.skip_frame
        self.is_wave = False
        self.use_cmvn = False
        # set (by the pipelined decoder, for the length of a decode) when the consumer applies the global CMVN itself, on the
        # device (pipeline.DecodePipelines(cmvn=...)): the fast path below then hands the features over as they are in the archive
        self.device_cmvn = False
        # --hip_segments: the utterances are sample ranges of the recordings the scp names (``data.segments``)
        seg_path = getattr(args, "hip_segments", "") or ""
        segs = segments.read_segments(seg_path) if seg_path else None
        self.data_streams = [SingleSet(vocab, p, getattr(args, "rank", 0), segs) for p in data_paths]
        self._items = [it for s in self.data_streams for it in s.items]
        self.seg_ranges = [r for s in self.data_streams for r in s.ranges] if segs is not None else None
        self.wave_ranges = self.segment_offsets = None
        self._maps = collections.OrderedDict()
        if segs is not None:
            segments.check_recordings(segs, [r for s in self.data_streams for r in s.recordings], seg_path)
        self.is_flac = False
        found = sniff_wave_set(self._items, getattr(args, "hip_audio", "auto"))
        if segs is not None and found is not True:
            raise ValueError("--hip_segments %s: %s" % (seg_path, "cutting segments out of FLAC files is not implemented (WAV recordings only)"
                                                        if found == "flac" else "the set is not audio: segments cut sample ranges out of WAV recordings"))
        if found:
            self._init_wave_set(args, flac=found == "flac")

    def _init_wave_set(self, args, flac=False):
        """A wave set: the entries are sound files, the dataset hands out (utt, int16 view, text) and the features are computed on
        the device by the consumer.  Every header is read once and checked here - format, rate and channels against what the
        front-end admits, at least one frame of the wave at the front-end's rate (``cn_resample_num_samples`` of the file's samples)
        - so that a bad file is named before anything is decoded.  ``wave_formats`` keeps each file's (rate, channels)."""
        if self.left_context != 0:
            raise NotImplementedError("audio input with left_ctx = %d (right_ctx >= 0 and skip_frame >= 1 are spliced on the device; a "
                                      "left context on audio input is not implemented)" % self.left_context)
        if self.right_context < 0 or self.skip_frame < 0:
            raise ValueError("audio input: right_ctx = %d, skip_frame = %d" % (self.right_context, self.skip_frame))
        fe = front_end(args)
        self.fbank_opts, self.wave_admit = fe.o, fe.admit()
        self.sample_rate, self.num_mel = float(self.fbank_opts.sample_rate), int(self.fbank_opts.num_mel)
        self.wave_frames, self.wave_formats = [], []
        own = int(round(self.sample_rate))
        self.flac_infos = [] if flac else None  # a FLAC set: per file its path and metadata (``flac_io.Info``), read once here
        headers = {}  # (--hip_segments: one look at a recording's header, however many segments it carries)
        if self.seg_ranges is not None:
            self.wave_ranges, self.segment_offsets = [], {}
        for k, (utt, spec, _) in enumerate(self._items):
            if flac:
                path = flac_io.flac_path(spec)
                info = flac_io.checked(path, self.sample_rate, utt, **self.wave_admit)
                # (a STREAMINFO total of 0 means unknown: the index says how many samples the frames hold)
                n, rate, channels = info.total or flac_io.frame_index(path, info, utt).samples, info.rate, info.channels
                self.flac_infos.append((path, info, n))
            elif self.seg_ranges is not None:
                rec, start, end = self.seg_ranges[k]
                if spec not in headers:
                    headers[spec] = wave_io.wave_format(spec, self.sample_rate, rec, **self.wave_admit)
                total, rate, channels = headers[spec]
                first, last = segments.sample_range(start, end, rate, total, utt, rec)
                n = last - first
                self.wave_ranges.append((first, last))
                self.segment_offsets[utt] = (rec, first / rate)
            else:
                n, rate, channels = wave_io.wave_format(spec, self.sample_rate, utt, **self.wave_admit)
            if rate != own:
                if self.sample_rate != own:
                    raise ValueError("utterance %s (%s): %d Hz, and resampling needs an integer --sample-frequency (it is %r)"
                                     % (utt, spec, rate, self.sample_rate))
                from .. import hip

                n = hip.resample_num_samples(rate, own, n)
            frames = frames_of(self.fbank_opts, n)
            if frames < 1:
                raise ValueError("%s (%s): %d samples%s give no frame (shorter than one analysis window)"
                                 % ("utterance %s" % utt if self.seg_ranges is None else "segment %s of recording %s" % (utt, self.seg_ranges[k][0]),
                                    spec, n, "" if rate == own else " at %d Hz (resampled from %d Hz)" % (own, rate)))
            self.wave_frames.append(frames)
            self.wave_formats.append((rate, channels))
        # (a set of mono files at the front-end's rate - every set there was before the options - hands out plain sample views)
        self.wave_plain = all(f == (own, 1) for f in self.wave_formats)
        self.is_wave = True
        self.is_flac = bool(flac)
        self._kinds = frozenset(["FLAC" if flac else "WAV"])

    def _load_cmvn(self, cmvn_file):
        """Kaldi global CMVN stats: row 0 = sums (last column = frame count), row 1 = sums of squares."""
        stats = kaldi_io.load_mat(cmvn_file)
        count = stats[0, -1]
        self.mean = stats[0, :-1] / count
        self.std = np.sqrt(stats[1, :-1] / count - self.mean ** 2)
        self.use_cmvn = True
        return 0

    def __len__(self):
        return len(self._items)

    def __getitem__(self, idx):
        utt, spec, text = self._items[idx]
        if self.is_flac:  # (the frames as the file holds them, with their exact index; decoded on the device)
            path, info, _ = self.flac_infos[idx]
            view = flac_io.audio_view(path, info)
            return utt, FlacFrames(view, flac_io.frame_index(path, info, utt, view)), text
        if self.is_wave and self.wave_ranges is not None:
            # (--hip_segments: the slice [first * channels, last * channels) of the recording's interleaved samples - for a mono file
            # at the front-end's rate the plain int16 pass -, from ONE memory map per recording, kept for the life of the dataset)
            view = self._maps.get(spec)
            if view is None:
                view = self._maps[spec] = wave_io.pcm_frames(spec, self.sample_rate, self.seg_ranges[idx][0], **self.wave_admit)[0]
                if len(self._maps) > MAX_SEGMENT_MAPS:  # (a map holds a file descriptor: the least recently used one goes)
                    self._maps.popitem(last=False)
            else:
                self._maps.move_to_end(spec)
            (first, last), channels = self.wave_ranges[idx], self.wave_formats[idx][1]
            return utt, view[first * channels:last * channels], text
        if self.is_wave:  # (the samples as the file holds them; normalisation happens with the features, on the device)
            if self.wave_plain:
                return utt, wave_io.pcm_view(spec, self.sample_rate, utt), text
            # (the interleaved data chunk; ``wave_formats[idx]`` says what it holds, resampling and the channel pick happen on the device)
            return utt, wave_io.pcm_frames(spec, self.sample_rate, utt, **self.wave_admit)[0], text
        if self.left_context == 0 and self.right_context == 0 and self.skip_frame <= 1:
            # No splicing, no frame skipping (the benchmark's configuration; the recipes' decode YAMLs splice - right_ctx 2 - and
            # take the general path below, or the packed reader's device splice).  Same values as the general path - the CMVN in
            # float64, rounded to float32 once (where the reference's collate converts: speech_loader.py:340) - without its
            # temporaries: the matrix is read in place from a memory map of the archive, the float64 intermediate lives in a
            # per-thread scratch buffer, and what is handed on is float32 (half the bytes for collate to move).
            feat = kaldi_io.load_mat_view(spec)
            if not self.use_cmvn or self.device_cmvn:
                return utt, feat, text
            assert feat.shape[1] == self.mean.shape[0]
            tmp = _scratch64(feat.shape)
            np.subtract(feat, self.mean, out=tmp)
            np.divide(tmp, self.std, out=tmp)
            return utt, tmp.astype(np.float32), text
        feat = kaldi_io.load_mat(spec)
        if self.use_cmvn:
            assert feat.shape[1] == self.mean.shape[0]
            feat = (feat - self.mean) / self.std
        rem = feat.shape[0] % self.skip_frame if self.skip_frame > 1 else 0
        if rem:
            feat = np.vstack([feat, np.zeros((self.skip_frame - rem, feat.shape[1]))])
        feat = skip_feat(context_feat(feat, self.left_context, self.right_context), self.skip_frame)
        return utt, feat, text

    def splice(self):
        """(left, right, skip) when the set splices or skips frames, None when it does neither."""
        return splice_triple(self.left_context, self.right_context, self.skip_frame)

    def device_splice(self):
        """The splice triple when the set splices or skips AND is otherwise what the packed reader takes - float32 (`FM `) or
        compressed (`CM` / `CM2` / `CM3`) matrices throughout, or sound files: CMVN, zero rows, splice and skip then happen on the
        device (``hip.splice_rows``), in the dataset's own order and arithmetic.  None for a set that does not splice, holds a
        float64 (`DM`) matrix or mixes the two families: those keep the host path.  ``can_defer_cmvn()`` is a different question
        (does the CMVN commute with what the HOST path does afterwards) and stays False for every spliced archive."""
        triple = self.splice()
        if triple is None:
            return None
        if self.is_wave:
            return triple
        kinds = self.matrix_kinds()
        return triple if (kinds <= {"FM"} or kinds <= set(kaldi_io.COMPRESSED_KINDS)) else None

    def can_defer_cmvn(self):
        """The global CMVN commutes with everything this dataset does afterwards (no splicing, no frame skipping) AND the archive
        holds float32 matrices: the device form computes float((double)x - mean) / std) on the float32 rows collate hands over,
        which is the reference's arithmetic bit for bit only when those rows are the archive's own values.  A float64 (`DM`)
        archive is normalised in float64 and rounded once (here, on the host, as the reference does).  Compressed matrices
        (`CM`, `CM2`, `CM3`) decompress to float32 values: they defer like `FM `.  A wave set always defers: its features exist on
        the device only."""
        if self.is_wave:
            return True
        if not (self.left_context == 0 and self.right_context == 0 and self.skip_frame <= 1):
            return False
        return "DM" not in self.matrix_kinds()

    def matrix_kinds(self):
        """The kinds of matrix this set holds (``kaldi_io.mat_kind``), from EVERY utterance's header: Kaldi mixes `CM` and `CM2`
        inside one archive, and a table may point into archives of different kinds.  A wave set (sound files) is {"WAV"}, a FLAC
        set {"FLAC"}."""
        if getattr(self, "_kinds", None) is None:
            self._kinds = frozenset(kaldi_io.mat_kind(spec) for _, spec, _ in self._items)
        return self._kinds


_tls = threading.local()


def _scratch64(shape):
    """float64 scratch of at least `shape` for the calling thread (grown by doubling, reused across utterances)"""
    n = int(shape[0]) * int(shape[1])
    buf = getattr(_tls, "buf", None)
    if buf is None or buf.size < n:
        buf = np.empty(max(n, 2 * (buf.size if buf is not None else 0)), dtype=np.float64)
        _tls.buf = buf
    return buf[:n].reshape(shape)


def collate(batch, padding_idx=0):
    """list of (utt, feat (T,F), text) -> (utts, feats (B,Tmax,F) f32, texts (B,L) i64, feat ratios (B,) f32,
    text sizes (B,) i64), padded with `padding_idx` exactly as the reference's SuperviseLoader.collate_fn.
    (Measured on the GPU box, 6000 ragged utterances: copying the rows on a small thread pool, or assembling the batch in page-locked
    memory, both made the recogniser slower than this plain loop - profiles/r04c_*.)"""
    t_max = max(x[1].shape[0] for x in batch)
    l_max = max(len(x[2]) for x in batch)
    feats = torch.empty((len(batch), t_max, batch[0][1].shape[1]))  # (every element is written below: rows, then padding tails)
    fv = feats.numpy()
    texts = torch.full((len(batch), l_max), int(padding_idx), dtype=torch.long)
    ratios = torch.zeros(len(batch))
    sizes = torch.zeros(len(batch), dtype=torch.long)
    utts = []
    for b, (utt, feat, text) in enumerate(batch):
        fv[b, : feat.shape[0]] = feat  # (numpy: a float64 matrix is rounded to float32 here, as torch.Tensor(feat) does; a read-only map is fine)
        if feat.shape[0] < t_max:
            fv[b, feat.shape[0] :] = float(padding_idx)
        texts[b, : len(text)] = torch.as_tensor(text, dtype=torch.long)
        ratios[b] = feat.shape[0] / t_max
        sizes[b] = len(text) - 2
        utts.append(utt)
    return utts, feats, texts, ratios, sizes


def collate_waves(batch, padding_idx=0, opts=None, splice=None, formats=None):
    """``collate`` for a wave set: list of (utt, int16 samples, text) -> the same five-tuple with a ``WaveBatch`` where the padded
    features would stand (no GPU is touched here: a loader worker process may run it).  With a ``splice`` triple the ratios are the
    spliced frame counts' (``spliced_frames``).  ``formats``: {utt: (rate, channels)} of a set that holds other files than mono ones
    at the front-end's rate (their samples are the interleaved data chunks; the frames are those of the resampled wave)."""
    index = None
    if formats is None:
        frames, fmts = [frames_of(opts, int(x[1].shape[0])) for x in batch], None
    else:
        from .. import hip

        own = int(round(float(opts.sample_rate)))
        fmts = [formats[x[0]] for x in batch]
        if isinstance(batch[0][1], FlacFrames):  # a FLAC set: the index rides beside the formats, the sample counts come from it
            index = [x[1].index for x in batch]
            batch = [(x[0], x[1].view, x[2]) for x in batch]
            per = [ix.samples for ix in index]
        else:
            per = [int(x[1].shape[0]) // c for x, (r, c) in zip(batch, fmts)]
        frames = [frames_of(opts, hip.resample_num_samples(r, own, n)) for n, (r, c) in zip(per, fmts)]
    n_out = [spliced_frames(n, splice) for n in frames]
    t_max = max(n_out)
    l_max = max(len(x[2]) for x in batch)
    texts = torch.full((len(batch), l_max), int(padding_idx), dtype=torch.long)
    ratios = torch.zeros(len(batch))
    sizes = torch.zeros(len(batch), dtype=torch.long)
    utts = []
    for b, (utt, _, text) in enumerate(batch):
        texts[b, : len(text)] = torch.as_tensor(text, dtype=torch.long)
        ratios[b] = n_out[b] / t_max
        sizes[b] = len(text) - 2
        utts.append(utt)
    return utts, WaveBatch([x[1] for x in batch], frames, opts.num_mel, utts, splice=splice, formats=fmts, index=index), texts, ratios, sizes


def _one_thread_worker(_worker_id):
    """A loader worker reads and pads a few megabytes: one thread.  Left at torch's default, every worker starts an intra-op
    team as wide as the machine whose idle threads spin - on a box with a CPU quota the whole job (the process that launches
    the kernels included) is then throttled for most of every scheduling period (measured: 11 s instead of 0.4 s for 6000
    utterances with four workers)."""
    torch.set_num_threads(1)


class SpeechDataLoader(DataLoader):
    def __init__(self, dataset, batch_size, padding_idx=-1, distributed=False, shuffle=False, num_workers=0, indices=None):
        if distributed or shuffle:
            raise NotImplementedError("training-time sampling is out of scope")
        self.padding_idx = padding_idx
        order = list(range(len(dataset))) if indices is None else list(indices)
        batches = [order[i : i + batch_size] for i in range(0, len(order), batch_size)]
        # worker processes hand their batches over in shared memory, from which a host -> device copy is pathologically slow
        # (83 ms per 9-MB batch measured): the loader's pinning thread moves them into page-locked memory first
        super().__init__(dataset, batch_sampler=batches, num_workers=num_workers,
                         collate_fn=(functools.partial(collate_waves, padding_idx=padding_idx, opts=dataset.fbank_opts, splice=dataset.splice(),
                                                       formats=None if dataset.wave_plain and not getattr(dataset, "is_flac", False) else
                                                       {it[0]: f for it, f in zip(dataset._items, dataset.wave_formats)})
                                     if getattr(dataset, "is_wave", False) else functools.partial(collate, padding_idx=padding_idx)),
                         pin_memory=bool(num_workers > 0 and torch.cuda.is_available()),
                         worker_init_fn=_one_thread_worker if num_workers > 0 else None,
                         persistent_workers=bool(num_workers > 0))
