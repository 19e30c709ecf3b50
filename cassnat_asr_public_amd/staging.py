"""The packed reader of the decode pipelines: ``PackedBatch`` - a batch the reader has NOT collated: archive rows, compressed
payloads or sound samples as the files hold them - and ``PackedStaging``, the one path by which ``pipeline.DecodePipelines`` takes
a pass of them to the device: gathered into page-locked memory, one DMA, then the form's own kernel (``hip.unpack_rows``,
``hip.unpack_compressed``, ``hip.fbank_packed`` / the resampler) and, for a set that splices or skips frames, ``hip.splice_rows``.
What differs between the three forms is the small description its ``_*_form`` function returns."""
from types import SimpleNamespace

import numpy as np
import torch

from . import hip


def _name(utts, b):
    """How ``PackedBatch``'s constructors name utterance b of a batch in their errors."""
    return "utterance %s" % (utts[b] if utts is not None else "#%d of the batch" % b)


class PackedBatch:
    """A batch the reader has NOT collated: the utterances' archive rows as they lie in the .ark - read-only float32 views (n_b, F)
    into the memory map of the archive (``data.kaldi_io.load_mat_view``) - in the batch's order.  It stands where the padded
    (B, T, F) tensor of ``SuperviseLoader.collate_fn`` (src/data/speech_loader.py:327-356) would: ``shape`` is that tensor's shape,
    ``ratios()`` its float32 length ratios.  The decode pipelines copy the rows of a whole engine pass back to back into page-locked
    memory (one straight memcpy per utterance, no padding), send them with one DMA and spread them over the padded batch on the
    device (``hip.unpack_rows``: padding and, when asked for, the global CMVN in float64 happen there).

    The COMPRESSED form (``from_payloads`` on Kaldi `CM` / `CM2` / `CM3` entries; ``kinds`` is then a list, otherwise None) keeps
    per utterance the payload as the archive holds it - a read-only uint8 view from min_value on (``data.kaldi_io.mat_payload``) -
    its kind (1 / 2 / 3) and its rows; shape, lengths and ratios come from the headers.  The pipelines stage the payloads as they
    are, a quarter of the float32 bytes, and ``hip.unpack_compressed`` decompresses on the device; ``padded()`` - host
    decompression with ``kaldi_io.decompress`` - is the definition of what it must produce.

    The WAVE form (``from_waves``; ``kinds`` is the string "wave") keeps per utterance a read-only '<i2' view of the samples inside the
    memory map of its sound file (``data.wave_io.pcm_view``); ``lens`` are the frame counts of the fbank front-end and ``shape`` the
    padded FEATURE shape.  The pipelines stage the samples as they are and ``hip.fbank_packed`` computes the features on the
    device; there is no host fbank in the product, so ``padded()`` and ``matrices()`` raise.  With ``formats`` - per utterance the
    file's (rate, channels) - the views hold the INTERLEAVED data chunks of files at other rates or of several channels, ``channel``
    is the one that is read, and ``lens`` count the frames of the wave at the front-end's rate: ``hip.wave_resample`` writes that
    wave on the device, ``hip.fbank_packed_f32`` reads it.

    The FLAC form (``from_waves(..., index=...)``; ``kinds`` is the string "flac") keeps per utterance a read-only uint8 view of its
    FLAC file from the first audio frame on and, in ``index``, the file's exact frame index (``data.flac_io.FlacIndex``); ``formats``
    are STREAMINFO's (rate, channels).  The pipelines stage the frames as they are - about half the bytes of the 16-bit PCM - and the
    pass's frame table; ``hip.flac_decode`` writes the interleaved int16 PCM into a scratch of the slot that is laid out as staged WAV
    data chunks are, and the wave form's launches read that.

    SPLICING (``splice`` = (left, right, skip), every form): the set splices and / or skips frames (the recipes' decode YAMLs:
    0 / 2 / 1).  ``lens`` stay the SOURCE rows and ``source_shape`` the unspliced (B, longest source count, F0); ``shape`` is what the
    dataset's general host path collates - (B, longest n_out, (left + right + 1) * F0) with n_out = ``out_lens`` = ceil(rows / skip) -
    and ``ratios()`` are n_out / longest n_out.  ``padded()`` applies the dataset's steps on the host (``speech_loader.splice_host``:
    CMVN in float64, zero rows up to a multiple of skip, ``feat_op.context_feat``, ``feat_op.skip_feat``, then padding): the
    definition ``hip.splice_rows`` is held to."""

    __slots__ = ("views", "lens", "shape", "dtype", "is_cuda", "kinds", "utts", "splice", "source_shape", "out_lens", "formats", "channel", "index")

    def __init__(self, views, utts=None, splice=None):
        self._init(views, None, [int(v.shape[0]) for v in views], None, utts, splice)

    def _init(self, views, kinds, lens, cols, utts, splice, formats=None, channel=-1, index=None):
        """Every slot, for the three constructors: ``lens`` are the source rows (frames), ``cols`` the unspliced feature width (None:
        the width of the views)."""
        from .data.speech_loader import splice_triple, spliced_frames

        self.views, self.kinds, self.lens, self.utts = views, kinds, lens, utts
        self.formats, self.channel, self.index = formats, channel, index
        self.dtype = torch.float32
        self.is_cuda = False
        self.splice = splice_triple(*splice) if splice else None
        self.shape = self.source_shape = (len(views), max(lens), int(views[0].shape[1] if cols is None else cols))
        self.out_lens = [spliced_frames(n, self.splice) for n in lens]
        if self.splice is not None:
            self.shape = (len(views), max(self.out_lens), (self.splice[0] + self.splice[1] + 1) * self.shape[2])
        return self

    @classmethod
    def from_payloads(cls, entries, utts=None, compressed=None, cols=None, splice=None):
        """``entries``: one ``kaldi_io.mat_payload`` tuple (kind, rows, cols, payload) per utterance - all `FM` (the float32 form,
        as ``PackedBatch(views)``) or all of the compressed kinds, which may mix.  Every header is checked: an entry of the other
        family (``compressed`` = True / False: the family the caller expects; None: the first entry's), of another column count
        (``cols``; None: the first entry's) or whose payload is not the size its header gives raises a ValueError that names the
        utterance - nothing is strided on a guess."""
        from .data.kaldi_io import COMPRESSED_KINDS

        if not entries:
            raise ValueError("PackedBatch: an empty batch")
        want_c = (entries[0][0] in COMPRESSED_KINDS) if compressed is None else bool(compressed)
        want_cols = int(entries[0][2]) if cols is None else int(cols)
        views, kinds, lens = [], [], []
        for b, (kind, rows, ncols, payload) in enumerate(entries):
            is_c = kind in COMPRESSED_KINDS
            if kind != "FM" and not is_c:
                raise ValueError("PackedBatch: %s holds a %r matrix, which the packed reader does not take" % (_name(utts, b), kind))
            if is_c != want_c:
                raise ValueError("PackedBatch: %s holds a %r matrix in a batch of %s ones" % (_name(utts, b), kind, "compressed" if want_c else "float32"))
            if int(ncols) != want_cols:
                raise ValueError("PackedBatch: %s has %d columns, the batch %d" % (_name(utts, b), ncols, want_cols))
            rows, ncols = int(rows), int(ncols)
            if not is_c:
                if rows < 0 or payload.nbytes != 4 * rows * ncols:
                    raise ValueError("PackedBatch: %s: payload of %d bytes for %d x %d float32" % (_name(utts, b), payload.nbytes, rows, ncols))
                views.append(payload.view("<f4").reshape(rows, ncols))
                continue
            need = 16 + {"CM": 8 * ncols + rows * ncols, "CM2": 2 * rows * ncols, "CM3": rows * ncols}[kind]
            if rows < 0 or payload.dtype != np.uint8 or payload.ndim != 1 or payload.nbytes != need:
                raise ValueError("PackedBatch: %s: payload of %d bytes for a %d x %d %s matrix (%d)" % (_name(utts, b), payload.nbytes, rows, ncols, kind, need))
            if tuple(np.frombuffer(payload[8:16].tobytes(), "<i4")) != (rows, ncols):  # (the device strides by the payload's own header)
                raise ValueError("PackedBatch: %s: the payload's header does not say %d x %d" % (_name(utts, b), rows, ncols))
            views.append(payload)
            kinds.append(COMPRESSED_KINDS[kind])
            lens.append(rows)
        if not want_c:
            return cls(views, utts, splice=splice)
        return cls.__new__(cls)._init(views, kinds, lens, want_cols, utts, splice)

    @classmethod
    def from_waves(cls, views, frames, num_mel, utts=None, splice=None, formats=None, channel=-1, index=None):
        """``views``: one '<i2', one-dimensional, C-contiguous array of samples per utterance; ``frames``: their frame counts under
        the front-end's options (``Fbank.num_frames``).  Anything else - and an utterance of zero frames - raises a ValueError that
        names the utterance.  ``formats``: per utterance (rate, channels) of its file - the view is then the interleaved data chunk
        (``wave_io.pcm_frames``), ``frames`` count the wave at the front-end's rate and ``channel`` (the front-end's `--channel`)
        must name a channel of every file that has more than one; None: mono files at the front-end's rate.
        ``index``: per utterance the ``flac_io.FlacIndex`` of a FLAC file - the views are then one-dimensional C-contiguous uint8
        arrays, the file's frames, ``formats`` (required) what STREAMINFO says, and every frame of the index must lie inside its view."""
        if not views:
            raise ValueError("PackedBatch: an empty batch")
        if len(frames) != len(views):
            raise ValueError("PackedBatch: %d frame counts for %d utterances" % (len(frames), len(views)))
        if formats is not None and len(formats) != len(views):
            raise ValueError("PackedBatch: %d (rate, channels) pairs for %d utterances" % (len(formats), len(views)))
        if index is not None and (formats is None or len(index) != len(views)):
            raise ValueError("PackedBatch: a FLAC batch needs one frame index and one (rate, channels) pair per utterance")
        for b, v in enumerate(views):
            if index is not None:
                fr = np.asarray(index[b].frames)
                if not isinstance(v, np.ndarray) or v.dtype != np.uint8 or v.ndim != 1 or not v.flags.c_contiguous:
                    raise ValueError("PackedBatch: %s: the FLAC frames must be a one-dimensional C-contiguous uint8 array" % _name(utts, b))
                if (fr.ndim != 2 or fr.shape[1] != 3 or fr.shape[0] < 1 or fr.dtype != np.int32 or int(fr[:, 0].min()) < 0 or int(fr[:, 1].min()) < 1
                        or int((fr[:, 0].astype(np.int64) + fr[:, 1]).max()) > v.shape[0] or int(index[b].samples) < 1):
                    raise ValueError("PackedBatch: %s: the frame index does not lie inside the %d bytes of the file's frames" % (_name(utts, b), v.shape[0]))
                if int(frames[b]) < 1:
                    raise ValueError("PackedBatch: %s: %d samples give no frame" % (_name(utts, b), int(index[b].samples)))
                rate, chans = int(formats[b][0]), int(formats[b][1])
                if rate < 1 or not 1 <= chans <= 8 or (chans > 1 and not 0 <= int(channel) < chans):
                    raise ValueError("PackedBatch: %s: (rate, channels) = (%d, %d), channel %d" % (_name(utts, b), rate, chans, int(channel)))
                continue
            if not isinstance(v, np.ndarray) or v.dtype != np.dtype("<i2") or v.ndim != 1 or not v.flags.c_contiguous:
                raise ValueError("PackedBatch: %s: the samples must be a one-dimensional C-contiguous '<i2' array (got %s)"
                                 % (_name(utts, b), "%s %s" % (getattr(v, "dtype", type(v).__name__), getattr(v, "shape", ""))))
            if int(frames[b]) < 1:
                raise ValueError("PackedBatch: %s: %d samples give no frame" % (_name(utts, b), v.shape[0]))
            if formats is not None:
                rate, chans = int(formats[b][0]), int(formats[b][1])
                if rate < 1 or chans < 1 or v.shape[0] % chans:
                    raise ValueError("PackedBatch: %s: %d int16 values at (rate, channels) = (%d, %d)" % (_name(utts, b), v.shape[0], rate, chans))
                if chans > 1 and not 0 <= int(channel) < chans:
                    raise ValueError("PackedBatch: %s: %d channels, channel %d is not one of them" % (_name(utts, b), chans, int(channel)))
        return cls.__new__(cls)._init(list(views), "wave" if index is None else "flac", [int(n) for n in frames], num_mel, utts, splice,
                                      None if formats is None else [(int(r), int(c)) for r, c in formats], int(channel),
                                      None if index is None else list(index))

    def ratios(self):
        """collate's ``ratios[b] = feat.shape[0] / t_max``: the Python (double) quotient rounded to float32 (of the rows the dataset
        hands out: the spliced counts when the batch splices)"""
        t_max = self.shape[1]
        return torch.tensor([n / t_max for n in self.out_lens], dtype=torch.float32)

    def matrices(self):
        """The utterances' float32 matrices on the host (the compressed form decompressed by ``kaldi_io.decompress``)."""
        if self.kinds is None:
            return self.views
        if self.kinds in ("wave", "flac"):
            raise NotImplementedError("PackedBatch: the wave form holds samples - the features exist on the device only (hip.fbank_packed)")
        from .data.kaldi_io import decompress

        names = {1: "CM", 2: "CM2", 3: "CM3"}
        return [decompress(names[k], n, self.source_shape[2], v) for k, n, v in zip(self.kinds, self.lens, self.views)]

    def padded(self, pad=0.0, cmvn=None):
        """The collated tensor itself (host): what the packed path must reproduce; used by the CPU rehearsal and the tests."""
        if self.kinds in ("wave", "flac"):
            raise NotImplementedError("PackedBatch: the wave form holds samples - the features exist on the device only (hip.fbank_packed)")
        out = np.full(self.shape, float(pad), np.float32)
        if self.splice is not None:
            from .data.speech_loader import splice_host

            for b, v in enumerate(self.matrices()):  # (the assignment rounds to float32 once, as collate does)
                out[b, : self.out_lens[b]] = splice_host(v, self.splice, cmvn)
            return torch.from_numpy(out)
        for b, v in enumerate(self.matrices()):
            out[b, : v.shape[0]] = v if cmvn is None else ((v.astype(np.float64) - cmvn[0]) / cmvn[1]).astype(np.float32)
        return torch.from_numpy(out)


def _form(f):
    """The staging form of a batch: None (a tensor, or float32 archive rows), "compressed", "wave" or "flac"."""
    kinds = getattr(f, "kinds", None)
    return None if kinds is None else (kinds if isinstance(kinds, str) else "compressed")


def _byte_layout(views, what, **rest):
    """The two forms staged as BYTES: every piece at a 16-byte-aligned offset of uint8 buffers, int32 offsets."""
    offs, total = hip.gather_offsets([v.nbytes for v in views], 16)
    if total >= 2 ** 31:
        raise ValueError("DecodePipelines: a pass of %d %s bytes (the offsets are int32)" % (total, what))
    return SimpleNamespace(dtype=torch.uint8, unit=1, gather={"align": 16}, offs=offs, total=total, fused=False, **rest)


class PackedStaging:
    """``DecodePipelines``' staging of a pass of ``PackedBatch``es (a mixin: ``_stage_packed`` reads ``_on_gpu``, ``_device`` and
    ``cmvn`` when it is called - all the CPU rehearsal needs - and, on the GPU, the pipelines' capacity, ``fbank``, ``copy_threads``,
    the per-pipeline buffer dicts ``_packed`` and the counters).

    A form's description (``_rows_form`` / ``_compressed_form`` / ``_wave_form``: its own checks, then a namespace) says: ``dtype`` and
    ``unit`` of the staging buffers (elements per unit of ``cap``), ``gather`` (the keywords of ``hip.host_gather``), ``offs`` and
    ``total`` (where the utterances lie, and the units the pass takes), ``cap`` (the units a slot is allocated with), ``col1`` and
    ``col3`` (per utterance, the small DMA's int32 columns 1 and - or None - 3; column 0 holds ``offs``, column 2 the float32 ratios),
    ``produce(bufs, m, out, stats)`` (the launch that writes the padded, normalised batch; ``m``: the columns on the device),
    ``fused`` (``hip.splice_rows`` reads the staging buffer itself - else the form produces into the slot's scratch first) and
    ``count`` (its counter)."""

    def _cmvn_stats(self, dev_):
        """The global CMVN's (mean, std) as float64 device tensors, uploaded at their first use - (None, None) without statistics."""
        if self.cmvn is None:
            return None, None
        stats = self._cmvn_dev.get(self._device)
        if stats is None:
            stats = self._cmvn_dev[self._device] = (torch.from_numpy(self.cmvn[0]).to(dev_), torch.from_numpy(self.cmvn[1]).to(dev_))
        return stats

    def _rows_form(self, batches, views, lens, area, utts, pad):
        """Float32 archive rows: a straight copy out of the memory map, offsets in ROWS, and ONE launch - ``hip.unpack_rows`` spreads
        the rows over the padded batch, or ``hip.splice_rows`` does that and the splice from the staging buffer."""
        offs = np.zeros(len(lens), np.int64)
        np.cumsum(lens[:-1], out=offs[1:])
        total = sum(lens)
        return SimpleNamespace(dtype=torch.float32, unit=batches[0].source_shape[2], gather={}, offs=offs, total=total, cap=max(total, area),
                               col1=lens, col3=None, fused=True, count=None,
                               produce=lambda bufs, m, out, stats: hip.unpack_rows(bufs["dev"], m[0], m[1], out, pad, *stats))

    def _compressed_form(self, batches, views, lens, area, utts, pad):
        """Kaldi `CM` / `CM2` / `CM3` payloads, mixed as they come, staged as the archive holds them - about a quarter of the float32
        bytes; their kinds ride in a fourth column and ``hip.unpack_compressed`` decompresses, normalises and pads.  Sized in bytes:
        area x F0 values of one byte plus the headers (grown for a pass that needs more, e.g. all `CM2`)."""
        F, F0 = batches[0].shape[2], batches[0].source_shape[2]
        if any(b.kinds is None or b.shape[2] != F for b in batches):
            raise ValueError("DecodePipelines: a pass mixes compressed and float32 packed batches, or feature dimensions")
        lay = _byte_layout(views, "compressed", count="compressed_passes", col1=lens, col3=[c for b in batches for c in b.kinds],
                           produce=lambda bufs, m, out, stats: hip.unpack_compressed(bufs["dev"], m[0], m[1], m[3], out, pad, *stats))
        lay.cap = max(lay.total, area * F0 + utts * (32 + 8 * F0))
        return lay

    def _wave_form(self, batches, views, lens, area, utts, pad, pcm=None):
        """int16 samples as the sound files hold them; the second column holds SAMPLES and ``hip.fbank_packed`` computes the padded
        features, normalised with the pipelines' statistics.  Sized in bytes: a frame shift of samples is 320 bytes at the default
        options, what 80 float32 features take.

        A pass that holds files at other rates or of several channels (``PackedBatch.formats``) stages the interleaved data chunks
        in the same buffers - sized in the bytes the files hold -, and one ``hip.wave_resample`` per distinct rate writes the chosen
        channel at the front-end's rate into the slot's float32 wave scratch, which ``hip.fbank_packed_f32`` reads
        (``data.fbank.plan_resample`` / ``run_resampled``; the resampler's per-utterance arrays travel in a small DMA of their own).
        A pass that needs neither is the int16 pass, launch for launch.

        ``pcm`` (the FLAC form): the samples are not the staged bytes but what ``hip.flac_decode`` wrote - a dict with the buffer's
        key in the slot (``src``), the utterances' byte ``offs`` and int16 counts (``lengths``) in it, its ``total`` bytes and
        ``cols`` (bufs -> the two device columns): the same launches then read that buffer."""
        from .data.fbank import RESAMPLE_META, plain_formats, plan_resample, run_resampled

        fb = self.fbank
        if fb is None:
            raise ValueError("DecodePipelines: a wave batch, but the pipelines were built without fbank options")
        F, F0 = batches[0].shape[2], batches[0].source_shape[2]
        if F0 != int(fb.num_mel) or any(b.shape[2] != F or b.source_shape[2] != F0 for b in batches):
            raise ValueError("DecodePipelines: wave batches of %d features, the front-end computes %d" % (F0, int(fb.num_mel)))
        own = int(round(float(fb.sample_rate)))
        formats = [f for b in batches for f in (b.formats if b.formats is not None else [(own, 1)] * len(b.views))]
        rates, chans = [r for r, _ in formats], [c for _, c in formats]
        resample = not plain_formats(fb.sample_rate, rates, chans)
        if resample and len(set(b.channel for b in batches if b.formats is not None)) > 1:
            raise ValueError("DecodePipelines: a pass mixes wave batches that read different channels")
        samples = [v.shape[0] for v in views] if pcm is None else pcm["lengths"]

        def produce(bufs, m, out, stats):
            src, total, offs = (bufs["dev"], lay.total, lay.offs) if pcm is None else (bufs[pcm["src"]], pcm["total"], pcm["offs"])
            if pcm is not None:
                m = pcm["cols"](bufs)
            if not resample:
                return hip.fbank_packed(fb, src, total, m[0], m[1], out, pad, *stats)
            U, dev_ = bufs["utts"], bufs["dev"].device
            if bufs.get("rs_h") is None:
                bufs["rs_h"] = torch.empty(RESAMPLE_META * U, dtype=torch.int32, pin_memory=True)
                bufs["rs_d"] = torch.empty(RESAMPLE_META * U, dtype=torch.int32, device=dev_)
            channel = next(b.channel for b in batches if b.formats is not None)
            plan = plan_resample(bufs["rs_h"].numpy(), U, fb, offs, samples, rates, chans, channel,
                                 [u for b in batches for u in (b.utts or [None] * len(b.views))])
            if bufs.get("wave") is None or bufs["wave"].numel() < plan["wave_floats"]:
                bufs["wave"] = torch.empty(max(plan["wave_floats"], bufs["cap"] // 2), dtype=torch.float32, device=dev_)
            bufs["rs_d"].copy_(bufs["rs_h"], non_blocking=True)
            run_resampled(fb, plan, src, total, bufs["rs_h"].numpy(), bufs["rs_d"], U, bufs["wave"], out, pad, *stats)
            self._bump("resampled_passes", 1)

        lay = _byte_layout(views, "sample", count="wave_passes", col1=samples, col3=None, produce=produce)
        shift = max(1, int(fb.sample_rate * 0.001 * fb.frame_shift_ms))
        flen = int(fb.sample_rate * 0.001 * fb.frame_length_ms)
        lay.cap = max(lay.total, 2 * area * shift + utts * (2 * flen + 16))
        return lay

    def _flac_form(self, batches, views, lens, area, utts, pad):
        """FLAC frames as the files hold them - about half the bytes of the 16-bit PCM - staged by the same gather and single DMA.
        The pass's frame table (``data.fbank.plan_flac``: per frame its byte offset, length, utterance and first sample - about 16
        bytes per 4096 samples - then per utterance channels, samples and the byte offset of its PCM, then the status word) follows
        in a DMA of its own; ``hip.flac_decode`` writes the interleaved int16 PCM into the slot's ``pcm`` scratch - sized from the
        headers, grown as ``bufs["wave"]`` is - at 16-byte-aligned offsets, exactly the staged data chunks of WAV files holding the
        same samples, and the wave form's ``produce`` (the resampled branch included) runs on that buffer.  The status word comes
        back with the results: ``_flac_checks`` holds, per slot, the check the pipelines make when the pass has drained."""
        from .data.fbank import flac_status_error, plan_flac

        if any(b.index is None for b in batches):
            raise ValueError("DecodePipelines: a pass mixes FLAC batches with another form of packed batch")
        chans = [c for b in batches for _, c in b.formats]
        names = [u for b in batches for u in (b.utts or [None] * len(b.views))]
        state = {}

        def cols(bufs):
            U, nf = bufs["utts"], state["nf"]
            return bufs["fl_d"][4 * nf + 2 * U:4 * nf + 3 * U], bufs["fl_d"][4 * nf + 3 * U + 1:4 * nf + 4 * U + 1]  # (PCM offsets, int16 counts)

        def produce(bufs, m, out, stats):
            U, dev_, B = bufs["utts"], bufs["dev"].device, len(views)
            nf = state["nf"] = plan["table"].shape[0]
            need = 4 * nf + 4 * U + 1  # the table; channels, samples, PCM offsets; the status word; the int16 counts
            if bufs.get("fl_h") is None or bufs["fl_h"].numel() < need:
                bufs["fl_h"] = torch.empty(2 * need, dtype=torch.int32, pin_memory=True)
                bufs["fl_d"] = torch.empty(2 * need, dtype=torch.int32, device=dev_)
                bufs["fl_back"] = torch.empty(1, dtype=torch.int32, pin_memory=True)
            fv = bufs["fl_h"].numpy()
            fv[:4 * nf] = plan["table"].ravel()
            for c in range(3):
                fv[4 * nf + c * U:4 * nf + c * U + B] = plan["utt"][c]
            fv[4 * nf + 3 * U] = 0
            fv[4 * nf + 3 * U + 1:4 * nf + 3 * U + 1 + B] = plan["lengths"]
            bufs["fl_d"][:need].copy_(bufs["fl_h"][:need], non_blocking=True)
            if bufs.get("pcm") is None or bufs["pcm"].numel() < plan["pcm_bytes"]:
                bufs["pcm"] = torch.empty(max(plan["pcm_bytes"], 2 * bufs["cap"]), dtype=torch.uint8, device=dev_)
            scratch = hip.flac_scratch_bytes(nf, plan["frame_words"])
            if bufs.get("fl_scratch") is None or bufs["fl_scratch"].numel() < scratch:
                bufs["fl_scratch"] = torch.empty(scratch + scratch // 4, dtype=torch.uint8, device=dev_)
            status = bufs["fl_d"][4 * nf + 3 * U:4 * nf + 3 * U + 1]
            hip.flac_decode(bufs["dev"], lay.total, bufs["fl_d"][:4 * nf], nf, bufs["fl_d"][4 * nf:4 * nf + 3 * U], U, plan["max_channels"],
                            plan["frame_words"], bufs["pcm"], plan["pcm_bytes"], status, bufs["fl_scratch"])
            bufs["fl_back"].copy_(status, non_blocking=True)
            back = bufs["fl_back"]

            def check():
                err = flac_status_error(int(back[0]), plan, names)
                if err is not None:
                    raise err

            state["check"] = check
            wave.produce(bufs, m, out, stats)
            self._bump("wave_passes", 1)

        lay = _byte_layout(views, "FLAC", count="flac_passes", col1=[v.shape[0] for v in views], col3=None, produce=produce)
        plan = plan_flac([ix for b in batches for ix in b.index], lay.offs, chans)
        wave = self._wave_form(batches, views, lens, area, utts, pad,
                               pcm={"src": "pcm", "offs": plan["pcm_offs"], "lengths": plan["lengths"], "total": plan["pcm_bytes"], "cols": cols})
        lay.cap = max(lay.total, wave.cap // 2)
        lay.state = state
        return lay

    def _stage_packed(self, k, slot, items, pad):
        """A pass of ``PackedBatch``es -> (the padded merged batch (rows, tmax, F), the float32 ratios), both on the device: every
        utterance's rows / payload / samples go into this slot's page-locked buffer (``hip.host_gather``: one GIL-free call - numpy's
        slice assignment holds the GIL, the pipelines' threads took turns; ``copy_threads`` > 1 deals the utterances over that many
        host threads inside it), ONE DMA takes them to the device, the per-utterance (offset, count, ratio as int32 bits[, kind])
        follow in one small DMA, and the form's kernel writes the batch - frames past an utterance's length get the padding value,
        and the global CMVN (float64, the dataset's arithmetic) is applied on the way when the pipelines have the statistics.  No
        padded batch ever exists on the host.  A spliced pass stages SOURCE rows of F0 values (skip times the output frames)."""
        on_gpu = self._on_gpu
        batches = [x[0] for x in items]
        rows = sum(b.shape[0] for b in batches)
        tmax = max(b.shape[1] for b in batches)
        F, F0, splice = batches[0].shape[2], batches[0].source_shape[2], batches[0].splice
        forms = set(_form(b) for b in batches)
        if len(set(b.splice for b in batches)) > 1:
            raise ValueError("DecodePipelines: a pass mixes packed batches of different splice triples")
        if "wave" in forms or "flac" in forms:
            if len(forms) > 1:
                raise ValueError("DecodePipelines: a pass mixes %s batches with another form of packed batch" % ("wave" if "flac" not in forms else "FLAC"))
            if not on_gpu:
                raise NotImplementedError("DecodePipelines: the wave form has no CPU rehearsal (the fbank front-end runs on the device only)")
        if not on_gpu:  # CPU rehearsal of the host logic: the collated tensors themselves
            feats = torch.full((rows, tmax, F), float(pad))
            o = 0
            for b in batches:
                feats[o:o + b.shape[0], : b.shape[1]] = b.padded(pad, self.cmvn)
                o += b.shape[0]
            return feats, torch.cat([x[1] for x in items], 0)
        dev_ = torch.device("cuda", self._device)
        form = _form(batches[0])
        views = [v for b in batches for v in b.views]
        lens = [n for b in batches for n in b.lens]
        area = self.max_batch * self.frames_cap
        want_utts = max(rows, self.max_utts)
        lay = {None: self._rows_form, "compressed": self._compressed_form, "wave": self._wave_form, "flac": self._flac_form}[form](
            batches, views, lens, area * (splice[2] if splice else 1), want_utts, pad)
        ncols = 3 + (lay.col3 is not None)
        # the slot's buffers, per form: allocated at the engines' area, again only for a pass that does not fit or another width
        bufs = self._packed[k].get((form, slot))
        if bufs is None or bufs["cap"] < lay.total or bufs["F"] != F or bufs["F0"] != F0 or bufs["utts"] < rows:
            bufs = {"cap": lay.cap, "F": F, "F0": F0, "utts": want_utts,
                    "host": torch.empty(lay.cap * lay.unit, dtype=lay.dtype, pin_memory=True),
                    "dev": torch.empty(lay.cap * lay.unit, dtype=lay.dtype, device=dev_),
                    "meta_h": torch.empty(ncols * want_utts, dtype=torch.int32, pin_memory=True),
                    "meta_d": torch.empty(ncols * want_utts, dtype=torch.int32, device=dev_),
                    "out": torch.empty(max(rows * tmax, area) * F, dtype=torch.float32, device=dev_)}
            self._packed[k][(form, slot)] = bufs
        if bufs["out"].numel() < rows * tmax * F:
            bufs["out"] = torch.empty(rows * tmax * F, dtype=torch.float32, device=dev_)
        hip.host_gather(bufs["host"].data_ptr(), views, max(1, self.copy_threads), **lay.gather)
        utts, meta = bufs["utts"], bufs["meta_h"].numpy()
        for c, col in enumerate([lay.offs, lay.col1, torch.cat([x[1] for x in items], 0).numpy().view(np.int32), lay.col3][:ncols]):
            meta[c * utts:c * utts + rows] = col
        n = lay.total * lay.unit
        bufs["dev"][:n].copy_(bufs["host"][:n], non_blocking=True)
        bufs["meta_d"].copy_(bufs["meta_h"], non_blocking=True)
        m = [bufs["meta_d"][c * utts:(c + 1) * utts] for c in range(ncols)]
        feats = bufs["out"][: rows * tmax * F].view(rows, tmax, F)
        stats = self._cmvn_stats(dev_)
        if splice is None:
            lay.produce(bufs, m, feats, stats)
        else:
            if lay.fused:  # padding, CMVN, zero rows, splice and skip in ONE launch from the staging buffer
                src, sp = bufs["dev"], (m[0], m[1])
            else:  # two launches: the form's kernel (with the CMVN) into the slot's scratch, then splice and skip out of it
                src, sp = self._splice_scratch(bufs, batches, rows, F0, splice, dev_)
                lay.produce(bufs, m, src, stats)
                stats = (None, None)
            hip.splice_rows(src, sp[0], sp[1], feats, splice[0], splice[1], splice[2], pad, *stats)
            self._bump("spliced_passes", 1)
        if lay.count:
            self._bump(lay.count, 1)
        if form == "flac":  # (the decoder's status word travels back behind the pass: checked when it has drained)
            self._flac_checks[k][slot] = lay.state["check"]
        return feats, m[2][:rows].view(torch.float32)

    def _splice_scratch(self, bufs, batches, rows, F0, splice, dev_):
        """The two-launch forms (compressed, wave) of a spliced pass: the slot's scratch for the UNSPLICED normalised batch - a
        (rows, T0, F0) view, T0 the pass's longest source count; allocated with the slot's other staging buffers at the size of the
        engines' area, grown only for a pass that needs more - and the per-utterance (row offset r * T0, source rows) that
        ``hip.splice_rows`` reads it by, sent in one small DMA.  Rows at or behind an utterance's count are never read there."""
        t0 = max(b.source_shape[1] for b in batches)
        need = rows * t0 * F0
        if bufs.get("mid") is None or bufs["mid"].numel() < need:
            bufs["mid"] = torch.empty(max(need, self.max_batch * self.frames_cap * splice[2] * F0), dtype=torch.float32, device=dev_)
        utts = bufs["utts"]
        if bufs.get("sp_h") is None:
            bufs["sp_h"] = torch.empty(2 * utts, dtype=torch.int32, pin_memory=True)
            bufs["sp_d"] = torch.empty(2 * utts, dtype=torch.int32, device=dev_)
        sp = bufs["sp_h"].numpy()
        sp[:rows] = np.arange(rows, dtype=np.int64) * t0
        sp[utts:utts + rows] = [n for b in batches for n in b.lens]
        bufs["sp_d"].copy_(bufs["sp_h"], non_blocking=True)
        return bufs["mid"][:need].view(rows, t0, F0), (bufs["sp_d"][:utts], bufs["sp_d"][utts:2 * utts])
