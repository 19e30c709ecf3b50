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
"""
import numpy as np
import torch

from .. import hip

WINDOWS = {"hamming": 0, "povey": 1, "hanning": 2, "rectangular": 3}
# Kaldi option (conf/fbank.conf: --name=value) -> (Fbank option, type)
CONF_OPTIONS = {"sample-frequency": ("sample_rate", float), "frame-length": ("frame_length_ms", float), "frame-shift": ("frame_shift_ms", float),
                "preemphasis-coefficient": ("preemph", float), "remove-dc-offset": ("remove_dc", bool), "window-type": ("window", str),
                "num-mel-bins": ("num_mel", int), "low-freq": ("low_freq", float), "high-freq": ("high_freq", float),
                "use-power": ("use_power", bool), "use-log-fbank": ("use_log", bool)}


def _conf_bool(name, text):
    if text.lower() not in ("true", "false"):
        raise ValueError("fbank conf: --%s=%s is not true / false" % (name, text))
    return text.lower() == "true"


def parse_conf(path):
    """A Kaldi option file (`--name=value` lines, blank lines, `#` comments) -> the keyword options of ``Fbank``.  `--use-energy=true`,
    `--snip-edges=false` and a non-zero `--dither` raise NotImplementedError (an absent `--dither` means 0: Kaldi's default adds
    noise and cannot be compared); an option this front-end does not know raises ValueError."""
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
                    opts[key] = kind(text)
            else:
                raise ValueError("fbank conf %s: unknown option --%s" % (path, name))
    return opts


class Fbank:
    def __init__(self, cmvn_mean=None, cmvn_std=None, pad_value=0.0, device=None, splice=None, **opts):
        """opts: sample_rate, frame_length_ms, frame_shift_ms, preemph, low_freq, high_freq, num_mel, window, remove_dc, ...
        ``splice`` = (left, right, skip): ``packed()`` splices and skips the normalised frames as the dataset does (``hip.splice_rows``)."""
        from .speech_loader import splice_triple

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

    def packed(self, views, utts=None):
        """``views``: one-dimensional int16 arrays (``wave_io.pcm_view``) -> (feats (B, T, num_mel) float32 cuda, ratios (B,) float32
        host) on the current stream.  The samples travel as they are - gathered at 16-byte-aligned offsets into page-locked memory,
        one copy - and ``hip.fbank_packed`` computes the padded batch on the device; no padded float matrix exists on the host."""
        frames = [self.num_frames(len(v)) for v in views]
        for b, n in enumerate(frames):
            if n < 1:
                raise ValueError("utterance %s: %d samples are shorter than one analysis window" % (utts[b] if utts is not None else "#%d" % b, len(views[b])))
        B, T = len(views), max(frames)
        views = [np.ascontiguousarray(v, dtype="<i2") for v in views]
        offs, total = hip.gather_offsets([v.nbytes for v in views], 16)
        if total >= 2 ** 31:
            raise ValueError("Fbank.packed: a batch of %d bytes (the offsets are int32)" % total)
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hip.host_gather(host.data_ptr(), views, 1, align=16)
        meta = torch.empty(2 * B, dtype=torch.int32, pin_memory=True)
        mv = meta.numpy()
        mv[:B] = offs
        mv[B:] = [len(v) for v in views]
        feats = torch.empty(B, T, self.o.num_mel, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            staged = host.to(self.device, non_blocking=True)
            meta_d = meta.to(self.device, non_blocking=True)
            hip.fbank_packed(self.o, staged, total, meta_d[:B], meta_d[B:], feats, self.pad_value, self.mean64, self.std64)
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
