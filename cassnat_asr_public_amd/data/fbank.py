"""Waveform -> padded log-mel filterbank batch on the GPU (csrc/fbank.hip through ``cn_fbank``).

The reference reads fbank features that Kaldi's ``compute-fbank-feats`` wrote (egs/librispeech/conf/fbank.conf:1-6) and
normalises them in ``SpeechDataset._load_cmvn`` (src/data/speech_loader.py:109-115); this module is that front-end for
callers that start from audio: ``Fbank()(waves) -> (feats (B, T, 80) float32 cuda, feat_sizes (B,) float32)`` in the
layout ``CassNAT.beam_decode`` takes (padded frames are exactly ``pad_value``; sizes are length ratios as the
reference's collate produces them, speech_loader.py:327-356).

``Fbank.packed(views)`` is the form the recogniser uses on a `wav.scp`: the utterances' int16 samples go to the device as the WAV
files hold them (``cn_host_gather`` into page-locked memory, one copy) and ``hip.fbank_packed`` computes the padded batch there, the
global CMVN in the dataset's float64 arithmetic.  ``Fbank.from_conf`` reads a Kaldi option file (conf/fbank.conf).  Dither is not
implemented: an absent ``--dither`` means 0 here, where Kaldi's default (1.0) adds noise that no two runs share.

Files at another sample rate or of several channels (``--allow-downsample`` / ``--allow-upsample`` / ``--channel``, the options of
compute-fbank-feats): ``packed(views, rates=..., channels=...)`` stages the interleaved int16 as it is, ``hip.wave_resample`` - Kaldi's
LinearResample, one launch per distinct rate - writes the chosen channel at ``sample_rate`` as float32, and ``hip.fbank_packed_f32``
computes the features from that.  A pass of mono files at ``sample_rate`` is the int16 path above, launch for launch.
"""
import numpy as np
import torch

from .. import hip

WINDOWS = {"hamming": 0, "povey": 1, "hanning": 2, "rectangular": 3}
# Kaldi option (conf/fbank.conf: --name=value) -> (Fbank option, type)
CONF_OPTIONS = {"sample-frequency": ("sample_rate", float), "frame-length": ("frame_length_ms", float), "frame-shift": ("frame_shift_ms", float),
                "preemphasis-coefficient": ("preemph", float), "remove-dc-offset": ("remove_dc", bool), "window-type": ("window", str),
                "num-mel-bins": ("num_mel", int), "low-freq": ("low_freq", float), "high-freq": ("high_freq", float),
                "use-power": ("use_power", bool), "use-log-fbank": ("use_log", bool),
                # not part of the option block: which files the front-end admits (attributes of ``Fbank``)
                "allow-downsample": ("allow_downsample", bool), "allow-upsample": ("allow_upsample", bool), "channel": ("channel", int)}
ADMIT_OPTIONS = {"allow_downsample": False, "allow_upsample": False, "channel": -1}


def _conf_bool(name, text):
    if text.lower() not in ("true", "false"):
        raise ValueError("fbank conf: --%s=%s is not true / false" % (name, text))
    return text.lower() == "true"


def parse_conf(path):
    """A Kaldi option file (`--name=value` lines, blank lines, `#` comments) -> the keyword options of ``Fbank``.  `--use-energy=true`,
    `--snip-edges=false` and a non-zero `--dither` raise NotImplementedError (an absent `--dither` means 0: Kaldi's default adds
    noise and cannot be compared); an option this front-end does not know raises ValueError.  `--allow-downsample`, `--allow-upsample`
    and `--channel` (a Kaldi config file may hold any command-line option of the program) come back as ``allow_downsample``,
    ``allow_upsample`` (0 / 1) and ``channel``."""
    opts = {}
    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            if not line.startswith("--") or "=" not in line:
                raise ValueError("fbank conf %s: not a --name=value line: %r" % (path, raw.rstrip("\n")))
            name, _, text = line[2:].partition("=")
            name, text = name.strip(), text.strip()
            if name == "use-energy":
                if _conf_bool(name, text):
                    raise NotImplementedError("fbank conf: --use-energy=true (an energy column) is not implemented")
            elif name == "snip-edges":
                if not _conf_bool(name, text):
                    raise NotImplementedError("fbank conf: --snip-edges=false is not implemented")
            elif name == "dither":
                if float(text) != 0.0:
                    raise NotImplementedError("fbank conf: --dither=%s: dither is not implemented (0 is what this front-end computes)" % text)
            elif name in CONF_OPTIONS:
                key, kind = CONF_OPTIONS[name]
                if kind is bool:
                    opts[key] = int(_conf_bool(name, text))
                elif kind is str:
                    if text not in WINDOWS:
                        raise ValueError("fbank conf: --window-type=%s (known: %s)" % (text, ", ".join(sorted(WINDOWS))))
                    opts[key] = text
                else:
                    try:
                        opts[key] = kind(text)
                    except ValueError:
                        raise ValueError("fbank conf: --%s=%s is not %s" % (name, text, "an integer" if kind is int else "a number"))
            else:
                raise ValueError("fbank conf %s: unknown option --%s" % (path, name))
    return opts


def plain_formats(sample_rate, rates, channels):
    """Does a pass need neither resampling nor a channel pick (every rate the front-end's, every file mono)?"""
    return (rates is None or all(int(r) == int(round(float(sample_rate))) for r in rates)) and (channels is None or all(int(c) == 1 for c in channels))


# int32 arrays of `utts` entries each in the small DMA of a resampled pass: byte offset, samples per channel, channels, channel,
# float offset of the resampled wave, its byte offset, its samples, the row lists of the rates (one after the other)
RESAMPLE_META = 8


def plan_resample(mv, U, opts, offs, lengths, rates, channels, channel, utts=None):
    """Host side of a resampled pass.  ``mv``: int32 numpy array of at least ``RESAMPLE_META * U`` entries (page-locked: it is the
    small DMA), filled here; ``offs`` / ``lengths``: per utterance the byte offset of the staged data chunk and its int16 values
    (all channels); ``channel``: the front-end's ``--channel``.  -> dict: ``counts`` (samples per utterance at the front-end's
    rate), ``wave_floats`` (the float32 wave buffer: utterance r at a multiple of 4 floats), ``groups`` [(rate, first entry of the
    row list, rows, longest output count)], ``out_rate``."""
    B = len(lengths)
    if float(opts.sample_rate) != int(round(float(opts.sample_rate))) or opts.sample_rate < 1:
        raise ValueError("fbank: resampling needs an integer --sample-frequency (it is %r)" % float(opts.sample_rate))
    fo = int(round(float(opts.sample_rate)))

    def name(b):
        return "utterance %s" % (utts[b] if utts is not None and utts[b] is not None else "#%d" % b)

    per, counts, chan = [], [], []
    for b in range(B):
        C = int(channels[b])
        if C < 1 or int(lengths[b]) % C:
            raise ValueError("%s: %d int16 values do not hold whole sample frames of %d channels" % (name(b), lengths[b], C))
        if C > 1 and not 0 <= int(channel) < C:
            raise ValueError("%s: %d channels, --channel=%d does not name one of them (set --channel to 0 .. %d)" % (name(b), C, channel, C - 1))
        if int(rates[b]) < 1:
            raise ValueError("%s: sample rate %d" % (name(b), rates[b]))
        per.append(int(lengths[b]) // C)
        chan.append(int(channel) if C > 1 else 0)
        counts.append(hip.resample_num_samples(int(rates[b]), fo, per[-1]))
    out_off = np.zeros(B, np.int64)
    np.cumsum([(n + 3) // 4 * 4 for n in counts[:-1]], out=out_off[1:])
    wave_floats = int(out_off[-1]) + (counts[-1] + 3) // 4 * 4
    if 4 * wave_floats >= 2 ** 31:
        raise ValueError("a pass of %d resampled float32 bytes (the offsets are int32)" % (4 * wave_floats))
    mv[:B] = offs
    mv[U:U + B] = per
    mv[2 * U:2 * U + B] = channels
    mv[3 * U:3 * U + B] = chan
    mv[4 * U:4 * U + B] = out_off
    mv[5 * U:5 * U + B] = out_off * 4
    mv[6 * U:6 * U + B] = counts
    groups, at = [], 0
    for rate in sorted(set(int(r) for r in rates)):
        rows = [b for b in range(B) if int(rates[b]) == rate]
        mv[7 * U + at:7 * U + at + len(rows)] = rows
        groups.append((rate, at, len(rows), max(counts[b] for b in rows)))
        at += len(rows)
    return {"counts": counts, "wave_floats": max(4, wave_floats), "groups": groups, "out_rate": fo, "B": B}


def run_resampled(opts, plan, staged, total, mv, meta_d, U, wave, feats, pad, mean=None, std=None):
    """Device side of a resampled pass, on the current stream: one ``hip.wave_resample`` per distinct rate over that rate's rows,
    then ``hip.fbank_packed_f32`` over the float32 wave.  ``mv`` / ``meta_d``: the array ``plan_resample`` filled and its device copy."""
    B = plan["B"]
    for rate, at, n, max_out in plan["groups"]:
        if max_out < 1:
            continue
        hip.wave_resample(rate, plan["out_rate"], staged, total, meta_d[:U], meta_d[U:2 * U], meta_d[2 * U:3 * U], meta_d[3 * U:4 * U],
                          mv[2 * U:2 * U + B], mv[3 * U:3 * U + B], wave, meta_d[4 * U:5 * U], max_out,
                          rows=meta_d[7 * U + at:7 * U + at + n], n_rows=n)
    hip.fbank_packed_f32(opts, wave, 4 * plan["wave_floats"], meta_d[5 * U:6 * U], meta_d[6 * U:7 * U], feats, pad, mean, std)


def plan_flac(index, offs, channels):
    """Host side of a FLAC pass.  ``index``: per utterance its ``flac_io.FlacIndex``; ``offs``: the byte offset of its frames in the
    staging buffer; ``channels``: its channel count.  -> dict: ``table`` int32 (frames, 4) - byte offset in the staging buffer, byte
    length, utterance, first sample -, ``utt`` int32 (3, B) - channels, samples per channel, byte offset of the PCM -, ``pcm_offs`` /
    ``pcm_bytes`` (every utterance's PCM at a 16-byte-aligned offset: the layout of staged WAV data chunks), ``lengths`` (int16
    values per utterance, all channels), ``frame_words`` and ``max_channels`` (what ``hip.flac_decode`` sizes its scratch by),
    ``starts`` (the first table row of every utterance)."""
    B = len(index)
    tabs, words, starts, at = [], 0, [], 0
    for b, ix in enumerate(index):
        fr = np.asarray(ix.frames, np.int32).reshape(-1, 3)
        if fr.shape[0] == 0:
            raise ValueError("utterance #%d: a FLAC index without frames" % b)
        t = np.empty((fr.shape[0], 4), np.int32)
        t[:, 0], t[:, 1], t[:, 2], t[:, 3] = fr[:, 0].astype(np.int64) + int(offs[b]), fr[:, 1], b, fr[:, 2]
        tabs.append(t)
        starts.append(at)
        at += fr.shape[0]
        longest = int(np.diff(np.append(fr[:, 2].astype(np.int64), int(ix.samples))).max())
        words = max(words, hip.flac_frame_words(int(channels[b]), max(1, longest)))
    lengths = [int(ix.samples) * int(c) for ix, c in zip(index, channels)]
    pcm_offs, pcm_bytes = hip.gather_offsets([2 * n for n in lengths], 16)
    if pcm_bytes >= 2 ** 31:
        raise ValueError("a pass of %d decoded PCM bytes (the offsets are int32)" % pcm_bytes)
    utt = np.empty((3, B), np.int32)
    utt[0], utt[1], utt[2] = channels, [int(ix.samples) for ix in index], pcm_offs
    return {"table": np.concatenate(tabs), "utt": utt, "pcm_offs": pcm_offs, "pcm_bytes": int(pcm_bytes), "lengths": lengths,
            "frame_words": words, "max_channels": int(max(channels)), "starts": starts}


def flac_status_error(status, plan, utts=None):
    """The status word of ``hip.flac_decode`` after a pass -> None (0: every frame decoded) or the ValueError that names the
    utterance and the frame.  With an index whose CRC-16s matched this does not happen; it is what keeps a wrong table from
    becoming a wild write."""
    if not status:
        return None
    f = int(status) - 1
    b = int(plan["table"][f, 2]) if 0 <= f < plan["table"].shape[0] else -1
    name = utts[b] if utts is not None and 0 <= b < len(utts) and utts[b] is not None else "#%d" % b
    return ValueError("utterance %s: FLAC frame %d (row %d of the pass's frame table) did not decode on the device: its bitstream does "
                      "not end on the frame's footer, or its block does not fit the utterance" % (name, f - plan["starts"][b] if b >= 0 else -1, f))


class Fbank:
    def __init__(self, cmvn_mean=None, cmvn_std=None, pad_value=0.0, device=None, splice=None, **opts):
        """opts: sample_rate, frame_length_ms, frame_shift_ms, preemph, low_freq, high_freq, num_mel, window, remove_dc, ...
        ``splice`` = (left, right, skip): ``packed()`` splices and skips the normalised frames as the dataset does (``hip.splice_rows``).
        ``allow_downsample`` / ``allow_upsample`` / ``channel`` (Kaldi's defaults: false, false, -1) say which files are admitted
        (``wave_io``); they are attributes, not part of the option block: ``key()`` does not see them."""
        from .speech_loader import splice_triple

        self.allow_downsample = bool(opts.pop("allow_downsample", ADMIT_OPTIONS["allow_downsample"]))
        self.allow_upsample = bool(opts.pop("allow_upsample", ADMIT_OPTIONS["allow_upsample"]))
        self.channel = int(opts.pop("channel", ADMIT_OPTIONS["channel"]))
        self.resampled_passes = self.flac_passes = 0
        self.splice = splice_triple(*splice) if splice else None
        self.L = hip.lib()
        self.o = hip.CnFbankOpts()
        self.L.cn_fbank_default_opts(self.o)
        if "window" in opts:
            opts["window_type"] = WINDOWS[opts.pop("window")]
        for k, v in opts.items():
            if not hasattr(self.o, k):
                raise TypeError(f"unknown fbank option {k}")
            setattr(self.o, k, v)
        if device is None:  # (without a GPU only the options and frame counts are of use: the dataset's header checks)
            self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        else:
            self.device = torch.device(device)
        self.pad_value = float(pad_value)
        self.mean = self.istd = self.mean64 = self.std64 = None
        if cmvn_mean is not None and self.device is not None:
            self.mean = torch.as_tensor(np.asarray(cmvn_mean, np.float32)).to(self.device)
            self.istd = torch.as_tensor((1.0 / np.asarray(cmvn_std, np.float64)).astype(np.float32)).to(self.device)
            # packed(): the dataset's arithmetic, float((double(e) - mean) / std)
            self.mean64 = torch.from_numpy(np.ascontiguousarray(cmvn_mean, dtype=np.float64)).to(self.device)
            self.std64 = torch.from_numpy(np.ascontiguousarray(cmvn_std, dtype=np.float64)).to(self.device)

    @classmethod
    def from_conf(cls, path, **kw):
        """The front-end a Kaldi option file describes (``parse_conf``); ``kw``: the other constructor arguments."""
        opts = parse_conf(path)
        opts.update(kw)
        return cls(**opts)

    def num_frames(self, num_samples):
        return int(self.L.cn_fbank_num_frames(self.o, int(num_samples)))

    def key(self):
        """The option block as bytes: what tells two front-ends apart."""
        return bytes(self.o)

    def admit(self):
        """The keyword options of ``wave_io`` that say which files this front-end takes."""
        return {"allow_downsample": self.allow_downsample, "allow_upsample": self.allow_upsample, "channel": self.channel}

    def packed(self, views, utts=None, rates=None, channels=None, flac=None):
        """``views``: one-dimensional int16 arrays (``wave_io.pcm_view``) -> (feats (B, T, num_mel) float32 cuda, ratios (B,) float32
        host) on the current stream.  The samples travel as they are - gathered at 16-byte-aligned offsets into page-locked memory,
        one copy - and ``hip.fbank_packed`` computes the padded batch on the device; no padded float matrix exists on the host.
        ``rates`` / ``channels``: per utterance the file's sample rate and channel count (``wave_io.pcm_frames``; the views then hold
        the interleaved data chunks).  None, or every rate equal to ``sample_rate`` and every file mono: exactly the path above.
        Otherwise the interleaved int16 is staged as it is (same gather, same single copy), one ``hip.wave_resample`` per distinct
        rate writes channel ``self.channel`` at ``sample_rate`` into a float32 wave buffer and ``hip.fbank_packed_f32`` reads that.
        The splice follows either way.
        ``flac``: per utterance the ``flac_io.FlacIndex`` of its file - ``views`` are then the files' uint8 frame bytes (``rates`` /
        ``channels`` from STREAMINFO are required): they are staged as they are, about half the bytes of the PCM, the pass's frame
        table follows in a DMA of its own and ``hip.flac_decode`` writes the interleaved int16 PCM into a device buffer laid out as
        the staged data chunks of WAV files would be - everything behind it is the path above, launch for launch."""
        resample = not plain_formats(self.o.sample_rate, rates, channels)
        B = len(views)
        if flac is not None:
            if rates is None or channels is None or len(flac) != B:
                raise ValueError("Fbank.packed: a FLAC batch needs one index, rate and channel count per utterance")
            views = [np.ascontiguousarray(v, dtype=np.uint8) for v in views]
        else:
            views = [np.ascontiguousarray(v, dtype="<i2") for v in views]
        offs, total = hip.gather_offsets([v.nbytes for v in views], 16)
        if total >= 2 ** 31:
            raise ValueError("Fbank.packed: a batch of %d bytes (the offsets are int32)" % total)
        counts, at = [v.shape[0] for v in views], ""  # (the samples the front-end sees, per utterance)
        if flac is not None:  # the front-end reads the decoded PCM: its offsets, its int16 counts
            fplan = plan_flac(flac, offs, [int(c) for c in channels])
            flac_offs, flac_total, offs, total, counts = offs, total, fplan["pcm_offs"], fplan["pcm_bytes"], fplan["lengths"]
        meta = torch.empty((RESAMPLE_META if resample else 2) * B, dtype=torch.int32, pin_memory=True)
        if resample:
            rates = [int(round(float(self.o.sample_rate)))] * B if rates is None else [int(r) for r in rates]
            channels = [1] * B if channels is None else [int(c) for c in channels]
            plan = plan_resample(meta.numpy(), B, self.o, offs, counts, rates, channels, self.channel, utts)
            counts, at = plan["counts"], " at %d Hz" % plan["out_rate"]
        else:
            meta.numpy()[:B], meta.numpy()[B:] = offs, counts
        frames = [self.num_frames(n) for n in counts]
        for b, n in enumerate(frames):
            if n < 1:
                raise ValueError("utterance %s: %d samples%s are shorter than one analysis window" % (utts[b] if utts is not None else "#%d" % b, counts[b], at))
        host = torch.empty(total if flac is None else flac_total, dtype=torch.uint8, pin_memory=True)
        hip.host_gather(host.data_ptr(), views, 1, align=16)
        feats = torch.empty(B, max(frames), self.o.num_mel, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            staged = host.to(self.device, non_blocking=True)
            meta_d = meta.to(self.device, non_blocking=True)
            if flac is not None:
                nf = fplan["table"].shape[0]
                fmeta = torch.empty(4 * nf + 3 * B + 1, dtype=torch.int32, pin_memory=True)
                fmeta.numpy()[:4 * nf], fmeta.numpy()[4 * nf:4 * nf + 3 * B], fmeta.numpy()[-1] = fplan["table"].ravel(), fplan["utt"].ravel(), 0
                fmeta_d = fmeta.to(self.device, non_blocking=True)
                pcm = torch.empty(max(16, total), dtype=torch.uint8, device=self.device)
                hip.flac_decode(staged, flac_total, fmeta_d[:4 * nf], nf, fmeta_d[4 * nf:4 * nf + 3 * B], B, fplan["max_channels"],
                                fplan["frame_words"], pcm, total, fmeta_d[-1:])
                err = flac_status_error(int(fmeta_d[-1].item()), fplan, utts)
                if err is not None:
                    raise err
                staged = pcm
                self.flac_passes += 1
            if resample:
                wave = torch.empty(plan["wave_floats"], dtype=torch.float32, device=self.device)
                run_resampled(self.o, plan, staged, total, meta.numpy(), meta_d, B, wave, feats, self.pad_value, self.mean64, self.std64)
                self.resampled_passes += 1
            else:
                hip.fbank_packed(self.o, staged, total, meta_d[:B], meta_d[B:], feats, self.pad_value, self.mean64, self.std64)
            return self._spliced(feats, frames)

    def _spliced(self, feats, frames):
        """The tail of ``packed``, inside its device context: (feats, ratios), spliced and skipped when the front-end has a triple."""
        B, T = feats.shape[0], feats.shape[1]
        if self.splice is None:
            return feats, torch.tensor([n / T for n in frames], dtype=torch.float32)
        # the set splices / skips: a second launch reads the normalised batch (utterance b at row b * T, its own frames only)
        from .speech_loader import spliced_frames

        left, right, skip = self.splice
        n_out = [spliced_frames(n, self.splice) for n in frames]
        sp = torch.empty(2 * B, dtype=torch.int32, pin_memory=True)
        spv = sp.numpy()
        spv[:B] = np.arange(B, dtype=np.int64) * T
        spv[B:] = frames
        sp_d = sp.to(self.device, non_blocking=True)
        out = torch.empty(B, max(n_out), (left + right + 1) * self.o.num_mel, dtype=torch.float32, device=self.device)
        hip.splice_rows(feats, sp_d[:B], sp_d[B:], out, left, right, skip, self.pad_value)
        return out, torch.tensor([n / max(n_out) for n in n_out], dtype=torch.float32)

    def __call__(self, waves):
        """waves: list of 1-D arrays / tensors on the int16 scale (what Kaldi reads from a wav file)."""
        ns = [int(len(w)) for w in waves]
        B, max_s = len(waves), max(ns)
        frames = [self.num_frames(n) for n in ns]
        T = max(frames)
        if T == 0:
            raise ValueError("every waveform is shorter than one analysis window")
        host = np.zeros((B, max_s), np.float32)
        for b, w in enumerate(waves):
            host[b, : ns[b]] = np.asarray(w.cpu() if isinstance(w, torch.Tensor) else w, dtype=np.float32)
        wave_d = torch.from_numpy(host).to(self.device)
        ns_d = torch.tensor(ns, dtype=torch.int32, device=self.device)
        feats = torch.empty(B, T, self.o.num_mel, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            hip.check(self.L.cn_fbank(self.o, hip._ptr(wave_d), hip._ptr(ns_d), B, max_s, hip._ptr(self.mean) if self.mean is not None else None,
                                      hip._ptr(self.istd) if self.istd is not None else None, hip._ptr(feats), T, self.pad_value,
                                      hip.current_stream()), "cn_fbank")
        sizes = torch.tensor([f / T for f in frames], dtype=torch.float32)
        return feats, sizes
