#!/usr/bin/env python3
"""Feature archives from audio - what Kaldi's `steps/make_fbank.sh` and `compute-cmvn-stats` give the recipes, written by this
project's own front end:

    python -m cassnat_asr_public_amd.bin.make_fbank --data_path data/test/wav.scp --out_dir data/fbank \\
        [--hip_fbank_conf conf/fbank.conf] [--compress true|false] [--batch_size 64] [--hip_audio auto|wav|flac] \\
        [--hip_compress device|host] [--hip_segments data/test/segments]

reads what `decode_asr` reads from audio (16-bit WAV, other rates and channels under the conf's --allow-* / --channel, FLAC) through
the same dataset and the packed reader's wave / FLAC forms (``staging.PackedStaging``: one gather, one DMA, the fbank kernel), and
writes

    DIR/feats.ark, DIR/feats.scp   `CM ` / `CM2 ` entries as `copy-feats --compress=true` chooses them, or `FM ` rows
                                   with --compress false; the scp in the wav.scp's order
    DIR/utt2num_frames
    DIR/cmvn.ark                   the global CMVN statistics of the values the archive holds (``SpeechDataset._load_cmvn`` reads it)

so that `decode_asr --data_path DIR/feats.scp --use_cmvn --global_cmvn DIR/cmvn.ark` decodes the set as often as a sweep needs it,
from a quarter of the float32 bytes.  Per pass: features on the device, ``hip.compress_feats``, ``hip.feats_stats``, then ONE copy of
stats, status words and payload bytes back to the host.  --hip_compress host brings the float32 rows back instead and runs the serial
twins of the two kernels (the comparison leg, and the fallback).  No model, no engine handle.  The archives hold UNSPLICED features:
left_ctx / right_ctx / skip_frame belong to the decoder.  A bad file or a non-zero status word ends the run naming the utterance;
everything is written under temporary names and renamed at the end, so a failed run leaves nothing behind.  With --hip_segments (a
Kaldi segments file over WAV recordings: ``data.segments``) the archives, utt2num_frames and the CMVN sums are per segment."""
import argparse
import collections
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from .. import hip
from ..data import kaldi_io
from ..staging import PackedBatch, PackedStaging

NAMES = ("feats.ark", "feats.scp", "utt2num_frames", "cmvn.ark")


class FeatureStager(PackedStaging):
    """The packed reader's wave and FLAC forms with no engine behind them: what ``pipeline.DecodePipelines`` gives the mixin, for one
    slot of one pipeline, without CMVN and without a splice."""

    def __init__(self, fbank_opts, batch_size, frames_cap=1024, device=None):
        import torch

        self.fbank, self.cmvn, self._cmvn_dev, self.copy_threads = fbank_opts, None, {}, 0
        self._packed, self._flac_checks = [{}], [{}]
        self.max_batch, self.frames_cap, self.max_utts = int(batch_size), int(frames_cap), int(batch_size)
        self._on_gpu = torch.cuda.is_available()
        self._device = (torch.cuda.current_device() if device is None else device) if self._on_gpu else None
        self.stats = collections.Counter()

    def _bump(self, key, v):
        self.stats[key] += v

    def features(self, batch):
        """A wave / FLAC ``PackedBatch`` -> (the padded (rows, Tmax, num_mel) float32 batch on the device, valid until the next call;
        the check of the FLAC decoder's status word, to be called once the stream has drained - or None)."""
        feats, _ = self._stage_packed(0, 0, [(batch, batch.ratios())], 0.0)
        return feats, self._flac_checks[0].pop(0, None)


class ArchiveWriter:
    """feats.ark / feats.scp / utt2num_frames / cmvn.ark of ``n`` utterances under temporary names, renamed by ``finish``.  Entries
    arrive in any order; the scp, utt2num_frames and the sums of the statistics follow the input order."""

    def __init__(self, out_dir, utts):
        os.makedirs(out_dir, exist_ok=True)
        self.out_dir, self.utts = out_dir, list(utts)
        self.final = {n: os.path.join(out_dir, n) for n in NAMES}
        self.tmp = {n: os.path.join(out_dir, ".%s.tmp%d" % (n, os.getpid())) for n in NAMES}
        self.offsets, self.frames, self.stats = [None] * len(self.utts), [0] * len(self.utts), [None] * len(self.utts)
        self.ark = open(self.tmp["feats.ark"], "wb")

    def add(self, i, frames, stats, mat=None, payload=None):
        """Utterance ``i`` of the input: its matrix (float32 rows) or its compressed payload, and its (2, F) sums."""
        entry, at = kaldi_io.matrix_entry(self.utts[i], mat=mat, payload=payload)
        self.offsets[i], self.frames[i], self.stats[i] = self.ark.tell() + at, int(frames), np.array(stats, np.float64)
        self.ark.write(entry)

    def finish(self):
        missing = [u for u, o in zip(self.utts, self.offsets) if o is None]
        if missing:
            raise ValueError("make_fbank: no features were written for utterance %s" % missing[0])
        self.ark.close()
        total = np.zeros_like(self.stats[0])
        for s in self.stats:  # (in input order: the same file whatever order the batches ran in)
            total += s
        with open(self.tmp["feats.scp"], "w") as f:
            for u, o in zip(self.utts, self.offsets):
                f.write("%s %s:%d\n" % (u, self.final["feats.ark"], o))
        with open(self.tmp["utt2num_frames"], "w") as f:
            for u, n in zip(self.utts, self.frames):
                f.write("%s %d\n" % (u, n))
        with open(self.tmp["cmvn.ark"], "wb") as f:
            f.write(kaldi_io.cmvn_stats_bytes(total[0], total[1], sum(self.frames)))
        for n in NAMES:
            os.replace(self.tmp[n], self.final[n])

    def abort(self):
        if not self.ark.closed:
            self.ark.close()
        for n in NAMES:
            if os.path.exists(self.tmp[n]):
                os.remove(self.tmp[n])


def batch_order(frames, batch_size, order="sorted"):
    """The utterances' indices in batches: "sorted" - longest first, so that a padded batch holds little padding; "input" - as they
    come; or a list of index lists (the tests shuffle)."""
    if not isinstance(order, str):
        return [list(b) for b in order]
    idx = sorted(range(len(frames)), key=lambda i: -frames[i]) if order == "sorted" else list(range(len(frames)))
    return [idx[i:i + batch_size] for i in range(0, len(idx), batch_size)]


def _status_error(utt, code):
    return ValueError("make_fbank: utterance %s: %s" % (utt, hip.FEATS_STATUS.get(int(code), "status %d" % int(code))))


def write_host(writer, idx, mats, compress):
    """The host leg of one batch: float32 matrices (one per utterance of ``idx``) through the serial twins of the two kernels."""
    F = mats[0].shape[1]
    lens = np.array([m.shape[0] for m in mats], np.int32)
    feats = np.zeros((len(mats), max(1, int(lens.max())), F), np.float32)
    for r, m in enumerate(mats):
        feats[r, :m.shape[0]] = m
    status = np.zeros(len(mats), np.int32)
    if not compress:
        stats = hip.feats_stats_host(feats, lens)
        for r, i in enumerate(idx):
            if lens[r] < 1 or not np.isfinite(mats[r]).all():
                raise _status_error(writer.utts[i], 1 if lens[r] < 1 else 2)
            writer.add(i, lens[r], stats[r], mat=np.ascontiguousarray(mats[r], np.float32))
        return feats.nbytes
    offs, sizes, total = hip.compress_feats_layout(lens, F)
    out = np.zeros(max(16, total), np.uint8)
    hip.compress_feats_host(feats, lens, offs, out, status)
    stats = hip.feats_stats_host(feats, lens, payload=out, out_off=offs, status=status)
    for r, i in enumerate(idx):
        if status[r]:
            raise _status_error(writer.utts[i], status[r])
        writer.add(i, lens[r], stats[r], payload=out[offs[r]:offs[r] + sizes[r]])
    return feats.nbytes


class DeviceLeg:
    """The device leg of a batch: compress and stats kernels behind the features, then one device-to-host copy of a buffer that
    holds the stats, the status words and the payloads (or, with --compress false, the stats and the padded float32 rows)."""

    def __init__(self):
        self.dev = self.host = self.meta_h = self.meta_d = None

    def _buffers(self, nbytes, rows, device):
        import torch

        if self.dev is None or self.dev.numel() < nbytes or self.dev.device != device:
            cap = nbytes + nbytes // 4
            self.dev = torch.empty(cap, dtype=torch.uint8, device=device)
            self.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        if self.meta_h is None or self.meta_h.numel() < 2 * rows or self.meta_d.device != device:
            self.meta_h = torch.empty(2 * max(rows, 64), dtype=torch.int32, pin_memory=True)
            self.meta_d = torch.empty(2 * max(rows, 64), dtype=torch.int32, device=device)

    def run(self, writer, idx, feats, lens, compress, check=None):
        import torch

        rows, tmax, F = feats.shape
        lens = np.asarray(lens, np.int32)
        n_stats = rows * 2 * F * 8
        at_status = n_stats
        at_data = (at_status + 4 * rows + 15) // 16 * 16
        if compress:
            offs, sizes, total = hip.compress_feats_layout(lens, F, tmax)
        else:
            offs, sizes, total = np.zeros(rows, np.int32), None, 4 * rows * tmax * F
        nbytes = at_data + max(16, total)
        self._buffers(nbytes, rows, feats.device)
        mv = self.meta_h.numpy()
        mv[:rows], mv[rows:2 * rows] = lens, offs
        self.meta_d[:2 * rows].copy_(self.meta_h[:2 * rows], non_blocking=True)
        d_lens, d_offs = self.meta_d[:rows], self.meta_d[rows:2 * rows]
        d_stats = self.dev[:n_stats].view(torch.float64).view(rows, 2, F)
        d_status = self.dev[at_status:at_status + 4 * rows].view(torch.int32)
        d_data = self.dev[at_data:at_data + max(16, total)]
        if compress:
            hip.compress_feats(feats, d_lens, d_offs, d_data, d_status)
            hip.feats_stats(feats, d_lens, d_stats, payload=d_data, out_off=d_offs, status=d_status)
        else:
            d_status.zero_()
            hip.feats_stats(feats, d_lens, d_stats)
            d_data[:total].view(torch.float32).copy_(feats.reshape(-1))
        self.host[:nbytes].copy_(self.dev[:nbytes], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        if check is not None:
            check()
        back = self.host.numpy()
        stats = back[:n_stats].view(np.float64).reshape(rows, 2, F)
        status = back[at_status:at_status + 4 * rows].view(np.int32)
        data = back[at_data:at_data + max(16, total)]
        for r, i in enumerate(idx):
            if compress:
                if status[r]:
                    raise _status_error(writer.utts[i], status[r])
                writer.add(i, lens[r], stats[r], payload=data[offs[r]:offs[r] + sizes[r]])
            else:
                mat = data[:total].view(np.float32).reshape(rows, tmax, F)[r, :lens[r]]
                if lens[r] < 1 or not np.isfinite(mat).all():
                    raise _status_error(writer.utts[i], 1 if lens[r] < 1 else 2)
                writer.add(i, lens[r], stats[r], mat=mat)
        return nbytes


def open_dataset(data_path, fbank_conf="", hip_audio="auto", segments=""):
    """The decoder's own dataset over the wav.scp (every header read and checked once: a bad or too short file is named here)."""
    from ..data.speech_loader import SpeechDataset

    args = SimpleNamespace(left_ctx=0, right_ctx=0, skip_frame=1, rank=0, hip_fbank_conf=fbank_conf or "",
                           hip_audio="auto" if hip_audio == "auto" else "1", hip_segments=segments or "")
    ds = SpeechDataset(None, [{"name": "make_fbank", "scp_path": data_path}], args)
    if not ds.is_wave:
        raise ValueError("make_fbank: %s does not name sound files (RIFF/WAVE or FLAC)" % data_path)
    if hip_audio != "auto" and (hip_audio == "flac") != bool(ds.is_flac):
        raise ValueError("make_fbank: --hip_audio %s, but %s holds %s files" % (hip_audio, data_path, "FLAC" if ds.is_flac else "WAV"))
    return ds


def packed_batch(ds, idx, pool=None):
    """The utterances ``idx`` of a wave / FLAC set as the packed reader's batch (what the pipelined decoder builds per batch)."""
    flac = bool(ds.is_flac)
    got = list(pool.map(ds.__getitem__, idx)) if (flac and pool is not None) else [ds[i] for i in idx]
    return PackedBatch.from_waves([v.view if flac else v for _, v, _ in got], [ds.wave_frames[i] for i in idx], ds.num_mel,
                                  utts=[u for u, _, _ in got], formats=None if ds.wave_plain and not flac else [ds.wave_formats[i] for i in idx],
                                  channel=ds.wave_admit["channel"], index=[v.index for _, v, _ in got] if flac else None)


def make_fbank(data_path, out_dir, fbank_conf="", compress=True, batch_size=64, hip_audio="auto", hip_compress="device", order="sorted",
               rows_of=None, segments=""):
    """The tool as a function -> a dict of counters (utterances, frames, passes, the bytes copied back from the device).
    ``rows_of`` (the host leg only): a callable (list of utterance names) -> their float32 matrices, in place of the device's
    features - the seam the host-logic tests use; the entries of ``data_path`` are then only names."""
    if hip_compress not in ("device", "host"):
        raise ValueError("make_fbank: --hip_compress is device or host")
    if rows_of is not None and segments:
        raise ValueError("make_fbank: --hip_segments cuts audio, rows_of stands in for it")
    if rows_of is not None and hip_compress != "host":
        raise ValueError("make_fbank: rows_of stands in for the device's features on the host leg only")
    if rows_of is None:
        ds = open_dataset(data_path, fbank_conf, hip_audio, segments)
        utts, frames = [it[0] for it in ds._items], list(ds.wave_frames)
    else:
        ds, utts = None, [u for u, _ in kaldi_io.read_scp(data_path)]
        frames = [0] * len(utts)
    if not utts:
        raise ValueError("make_fbank: %s lists no utterance" % data_path)
    if len(set(utts)) != len(utts):
        raise ValueError("make_fbank: %s names an utterance twice" % data_path)
    writer = ArchiveWriter(out_dir, utts)
    counters = collections.Counter(utterances=len(utts))
    pool = ThreadPoolExecutor(max_workers=4, thread_name_prefix="flac-index") if ds is not None and ds.is_flac else None
    try:
        stager = FeatureStager(ds.fbank_opts, batch_size) if ds is not None else None
        leg = DeviceLeg()
        for idx in batch_order(frames, int(batch_size), order):
            if rows_of is not None:
                mats = [np.asarray(m, np.float32) for m in rows_of([utts[i] for i in idx])]
                counters["bytes_back"] += write_host(writer, idx, mats, compress)
            else:
                pb = packed_batch(ds, idx, pool)
                feats, check = stager.features(pb)
                if hip_compress == "device":
                    counters["bytes_back"] += leg.run(writer, idx, feats, pb.lens, compress, check)
                else:
                    host = feats.cpu()  # (waits for the stream)
                    if check is not None:
                        check()
                    counters["bytes_back"] += write_host(writer, idx, [host[r, :n].numpy() for r, n in enumerate(pb.lens)], compress)
            counters["passes"] += 1
        writer.finish()
    except BaseException:
        writer.abort()
        raise
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
    counters["frames"] = sum(writer.frames)
    return dict(counters)


def main(argv=None):
    p = argparse.ArgumentParser(description="fbank feature archives and global CMVN statistics from a wav.scp, computed and compressed on the device")
    p.add_argument("--data_path", required=True, help="wav.scp: `UTT path` lines naming 16-bit WAV or FLAC files (what decode_asr reads from audio)")
    p.add_argument("--out_dir", required=True, help="receives feats.ark, feats.scp, utt2num_frames and cmvn.ark")
    p.add_argument("--hip_fbank_conf", default="", help="Kaldi option file of the front end (decode_asr's --hip_fbank_conf)")
    p.add_argument("--compress", default="true", choices=["true", "false"], help="true (default): `CM` / `CM2` entries; false: float32 `FM ` rows")
    p.add_argument("--batch_size", default=64, type=int, help="utterances per pass")
    p.add_argument("--hip_audio", default="auto", choices=["auto", "wav", "flac"], help="what the entries must be (auto: WAV or FLAC, found from the files)")
    p.add_argument("--hip_compress", default="device", choices=["device", "host"],
                   help="device (default): compression and statistics by the kernels behind the fbank kernel; host: the float32 rows come "
                        "back and the serial twins run (the comparison leg and the fallback)")
    p.add_argument("--hip_segments", default="", help="a Kaldi segments file (`UTT REC START END`): the utterances are sample ranges of the WAV "
                                                      "recordings --data_path names (decode_asr's --hip_segments)")
    a = p.parse_args(argv)
    if a.batch_size < 1:
        p.error("--batch_size must be at least 1")
    c = make_fbank(a.data_path, a.out_dir, a.hip_fbank_conf, a.compress == "true", a.batch_size, a.hip_audio, a.hip_compress,
                   segments=a.hip_segments)
    print("make_fbank: %d utterances, %d frames in %d passes -> %s" % (c["utterances"], c["frames"], c["passes"], a.out_dir))
    return 0


if __name__ == "__main__":
    sys.exit(main())
