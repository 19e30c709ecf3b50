#!/usr/bin/env python3
"""A Kaldi `segments` file from long recordings - what `compute-vad-decision` plus a segmentation script give a data directory -
by an energy VAD whose per-sample work runs on the device:

    python -m cassnat_asr_public_amd.bin.make_segments --data_path data/rec/wav.scp --out_dir data/rec \\
        [--hip_fbank_conf conf/fbank.conf] [--vad_conf conf/vad.conf] [--min_silence 0.3] [--min_speech 0.2] [--pad 0.1] \\
        [--max_segment 30] [--chunk_frames 60000] [--hip_vad device|host]

reads 16-bit WAV recordings of any rate (the VAD runs at each file's own rate: nothing is resampled) and writes

    DIR/segments            `REC-%08d-%08d REC %.3f %.3f`: the ids are the two times in milliseconds
    DIR/vad.scp, DIR/vad.ark   the per-frame decisions as a Kaldi float vector per recording, for inspection

so that `decode_asr --data_path wav.scp --hip_segments DIR/segments` decodes the recordings utterance by utterance.
--hip_fbank_conf gives the frame length and shift in ms, --remove-dc-offset and --channel; --vad_conf is Kaldi's option file of
compute-vad-decision (``utils.vad.parse_vad_conf``).  A recording is split into rows of at most --chunk_frames frames - row k covers the
frames [k C, min((k + 1) C, T)), that is the samples [k C shift, (last frame) shift + N) - so a recording of any length passes through a
bounded page-locked staging buffer (``hip.host_gather``, ONE host-to-device copy per pass) and its frame indices stay contiguous on the
device.  Per pass: ``hip.frame_energy``; after a recording's last chunk ``hip.vad_decide``; then e (8 bytes per frame) and dec (1 byte
per frame) come back and ``utils.vad.segment`` cuts the runs.  --hip_vad host runs the serial twins of the two entry points instead
and needs no GPU.  FLAC files, and a file whose frame length exceeds 2048 samples at its rate, are refused by name.  A recording without
speech writes no segment and is named on stderr.  Everything is written under temporary names and renamed at the end."""
import argparse
import collections
import os
import struct
import sys

import numpy as np

from .. import hip
from ..data import flac_io, kaldi_io, wave_io
from ..utils import vad

NAMES = ("segments", "vad.scp", "vad.ark")
MAX_N, MAX_CHANNELS = 2048, 8
PASS_BYTES = 64 << 20  # staged bytes of one pass (a single chunk larger than this is a pass of its own)
PASS_ROWS = 65535      # rows of one pass: what the entry points take in a call (and so the recordings of one decision)
COPY_THREADS = 4       # of the gather into the staging buffer

Recording = collections.namedtuple("Recording", "utt path samples rate channels N shift frames")
Chunk = collections.namedtuple("Chunk", "rec first_frame frames first_sample samples")


def front_end(fbank_conf):
    """(frame length ms, frame shift ms, remove_dc, channel) of --hip_fbank_conf (default: the built-in front end's)."""
    from ..data.fbank import Fbank

    fe = Fbank.from_conf(fbank_conf) if fbank_conf else Fbank()
    return float(fe.o.frame_length_ms), float(fe.o.frame_shift_ms), bool(fe.o.remove_dc), int(fe.channel)


def open_recordings(data_path, length_ms, shift_ms, channel):
    """Every header read and checked once -> [Recording]; a bad entry is named before anything runs."""
    out, seen = [], set()
    for utt, spec in kaldi_io.read_scp(data_path):
        if utt in seen:
            raise ValueError("make_segments: %s names recording %s twice" % (data_path, utt))
        seen.add(utt)
        if flac_io.is_flac(spec):
            raise ValueError("make_segments: recording %s (%s) is a FLAC stream: the VAD reads 16-bit WAV files only" % (utt, spec))
        path = wave_io.check_spec(spec, utt)
        n, rate, channels = wave_io.wave_format(path, None, utt, channel=channel)
        if channels > MAX_CHANNELS:
            raise ValueError("make_segments: recording %s (%s): %d channels (at most %d)" % (utt, path, channels, MAX_CHANNELS))
        N, shift = int(rate * 0.001 * length_ms), int(rate * 0.001 * shift_ms)
        if N > MAX_N:
            raise ValueError("make_segments: recording %s (%s): a frame of %g ms is %d samples at %d Hz, the VAD takes at most %d "
                             "(a shorter --frame-length)" % (utt, path, length_ms, N, rate, MAX_N))
        if N < 1 or shift < 1:
            raise ValueError("make_segments: recording %s (%s): frame length / shift of %d / %d samples at %d Hz" % (utt, path, N, shift, rate))
        out.append(Recording(utt, path, n, rate, channels, N, shift, 0 if n < N else 1 + (n - N) // shift))
    if not out:
        raise ValueError("make_segments: %s lists no recording" % data_path)
    return out


def plan_passes(recs, chunk_frames, pass_bytes=PASS_BYTES, pass_rows=PASS_ROWS):
    """-> [pass], a pass a list of ``Chunk``s of recordings that share (N, shift, channels), in input order, of at most ``pass_bytes``
    staged bytes (each chunk at a multiple of 16) and ``pass_rows`` chunks; a chunk whose bytes the int32 offsets cannot address is
    refused by name; and the frames the device buffers must hold: a recording's frames lie contiguously
    from the position it was given when its first chunk was planned, a recording that spans passes keeps its place, and the positions
    start again at 0 after a pass that leaves no recording open."""
    passes, cur, cur_bytes, key = [], [], 0, None
    for i, r in enumerate(recs):
        for k in range(0, r.frames, chunk_frames):
            frames = min(chunk_frames, r.frames - k)
            samples = (frames - 1) * r.shift + r.N
            nbytes = (samples * r.channels * 2 + 15) // 16 * 16
            if nbytes >= 2 ** 31:
                raise ValueError("make_segments: recording %s (%s): a chunk of %d frames is %d bytes, the staging offsets are int32 "
                                 "(a smaller --chunk_frames)" % (r.utt, r.path, frames, nbytes))
            if cur and (key != (r.N, r.shift, r.channels) or cur_bytes + nbytes > pass_bytes or len(cur) >= pass_rows):
                passes.append(cur)
                cur, cur_bytes = [], 0
            key = (r.N, r.shift, r.channels)
            cur.append(Chunk(i, k, frames, k * r.shift, samples))
            cur_bytes += nbytes
    if cur:
        passes.append(cur)
    places = place_per_pass(recs, passes)
    cap = max([at + recs[i].frames for place in places for i, at in place.items()] or [0])
    return passes, places, cap


def place_per_pass(recs, passes):
    """Per pass {recording: first index of its frames in the device buffers} (the rule ``plan_passes`` describes)."""
    out, place, fill = [], {}, 0
    for p in passes:
        for c in p:
            if c.rec not in place:
                place[c.rec] = fill
                fill += recs[c.rec].frames
        out.append(dict((c.rec, place[c.rec]) for c in p))
        last = p[-1]
        if last.first_frame + last.frames == recs[last.rec].frames:
            place, fill = {}, 0
        else:
            place = {last.rec: place[last.rec]}
            fill = place[last.rec] + recs[last.rec].frames
    return out


class HostLeg:
    """The serial twins: staging in ordinary memory, ``hip.frame_energy_host`` / ``hip.vad_decide_host``.  No GPU call."""

    def __init__(self, cap_frames, cap_bytes):
        self.staged = np.zeros(max(16, cap_bytes), np.uint8)
        self.num, self.e = np.zeros(max(1, cap_frames), np.int64), np.zeros(max(1, cap_frames), np.float64)
        self.dec = np.zeros(max(1, cap_frames), np.uint8)

    def energy(self, views, off, samples, out_off, total, r, remove_dc, channel, max_frames):
        hip.host_gather(self.staged.ctypes.data, views, COPY_THREADS, align=16)
        hip.frame_energy_host(self.staged, off, samples, out_off, r.N, r.shift, r.channels, channel, remove_dc, max_frames, self.num, self.e,
                              staged_bytes=total)

    def decide(self, rec_off, rec_frames, o):
        thr = np.zeros(rec_off.size, np.float64)
        hip.vad_decide_host(self.e, rec_off, rec_frames, o["thr0"], o["mean_scale"], o["context"], o["proportion"], thr, self.dec)
        return [(self.e[a:a + n].copy(), self.dec[a:a + n].copy()) for a, n in zip(rec_off, rec_frames)]


class DeviceLeg:
    """The kernels: chunks gathered into page-locked memory with their three int32 columns behind them, ONE host-to-device copy per
    pass, ``hip.frame_energy``; ``hip.vad_decide`` for the recordings a pass completes, then e and dec of those come back."""

    def __init__(self, cap_frames, cap_bytes, max_rows, max_recs):
        import torch

        self.torch = torch
        dev = torch.device("cuda", torch.cuda.current_device())
        nbytes = (max(16, cap_bytes) + 15) // 16 * 16 + 4 * 3 * max_rows
        self.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        n = max(1, cap_frames)
        self.num, self.e = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        self.dec = torch.empty(n, dtype=torch.uint8, device=dev)
        self.thr = torch.empty(max(1, max_recs) * (1 + hip.VAD_PARTS), dtype=torch.float64, device=dev)
        self.rmeta_h = torch.empty(2 * max(1, max_recs), dtype=torch.int32, pin_memory=True)
        self.rmeta_d = torch.empty(2 * max(1, max_recs), dtype=torch.int32, device=dev)

    def energy(self, views, off, samples, out_off, total, r, remove_dc, channel, max_frames):
        rows = off.size
        hip.host_gather(self.host.data_ptr(), views, COPY_THREADS, align=16)
        # the three columns stand right behind this pass's staged bytes (at the next multiple of 16): one copy takes both
        at = (int(total) + 15) // 16 * 16
        end = at + 12 * rows
        self.host.numpy()[at:end].view(np.int32)[:] = np.concatenate((off, samples, out_off))
        self.dev[:end].copy_(self.host[:end], non_blocking=True)
        m = self.dev[at:end].view(self.torch.int32)
        hip.frame_energy(self.dev, total, m[:rows], m[rows:2 * rows], m[2 * rows:], rows, r.N, r.shift, r.channels, channel, remove_dc, max_frames,
                         self.num, self.e)
        # (the page-locked buffer is filled again by the next pass: the copy must have left it)
        self.torch.cuda.current_stream().synchronize()

    def decide(self, rec_off, rec_frames, o):
        n = rec_off.size
        mv = self.rmeta_h.numpy()
        mv[:n], mv[n:2 * n] = rec_off, rec_frames
        self.rmeta_d[:2 * n].copy_(self.rmeta_h[:2 * n], non_blocking=True)
        hip.vad_decide(self.e, self.rmeta_d[:n], self.rmeta_d[n:2 * n], n, o["thr0"], o["mean_scale"], o["context"], o["proportion"], self.thr, self.dec)
        return [(self.e[a:a + k].cpu().numpy(), self.dec[a:a + k].cpu().numpy()) for a, k in zip(rec_off.tolist(), rec_frames.tolist())]


def vector_entry(key, values):
    """One entry of a binary Kaldi archive holding a float vector, and the offset of its binary marker inside the entry."""
    v = np.ascontiguousarray(values, "<f4")
    head = key.encode() + b" "
    return head + b"\0BFV \x04" + struct.pack("<i", v.size) + v.tobytes(), len(head)


def segment_lines(r, runs):
    out = []
    for a, b in runs:
        start = a * r.shift / r.rate
        end = min(((b - 1) * r.shift + r.N) / r.rate, r.samples / r.rate)
        out.append("%s-%08d-%08d %s %.3f %.3f\n" % (r.utt, int(round(start * 1000)), int(round(end * 1000)), r.utt, start, end))
    return out


def make_segments(data_path, out_dir, fbank_conf="", vad_conf="", min_silence=0.3, min_speech=0.2, pad=0.1, max_segment=30.0,
                  chunk_frames=60000, hip_vad="device", pass_bytes=PASS_BYTES, pass_rows=PASS_ROWS):
    """The tool as a function -> a dict of counters (recordings, frames, segments, passes, silent recordings)."""
    if hip_vad not in ("device", "host"):
        raise ValueError("make_segments: --hip_vad is device or host")
    if int(chunk_frames) < 1:
        raise ValueError("make_segments: --chunk_frames must be at least 1")
    length_ms, shift_ms, remove_dc, channel = front_end(fbank_conf)
    opts = vad.parse_vad_conf(vad_conf)
    recs = open_recordings(data_path, length_ms, shift_ms, channel)
    shift_sec = shift_ms * 0.001
    lens = [vad.frames_of_seconds(s, shift_sec) for s in (min_silence, min_speech, pad, max_segment)]
    if lens[3] < 2:
        raise ValueError("make_segments: --max_segment %g s is %d frames (at least 2)" % (max_segment, lens[3]))
    passes, places, cap_frames = plan_passes(recs, int(chunk_frames), min(int(pass_bytes), 2 ** 31 - 16), int(pass_rows))
    cap_bytes = max([sum((c.samples * recs[c.rec].channels * 2 + 15) // 16 * 16 for c in p) for p in passes] or [16])
    max_rows = max([len(p) for p in passes] or [1])
    leg = HostLeg(cap_frames, cap_bytes) if hip_vad == "host" else DeviceLeg(cap_frames, cap_bytes, max_rows, max_rows)
    os.makedirs(out_dir, exist_ok=True)
    final = {n: os.path.join(out_dir, n) for n in NAMES}
    tmp = {n: os.path.join(out_dir, ".%s.tmp%d" % (n, os.getpid())) for n in NAMES}
    counters = collections.Counter(recordings=len(recs), frames=sum(r.frames for r in recs), passes=len(passes))
    results, maps = {}, {}
    try:
        for p, place in zip(passes, places):
            r0 = recs[p[0].rec]
            views = []
            for c in p:
                r = recs[c.rec]
                if c.rec not in maps:  # (one memory map per recording, dropped with its last chunk)
                    maps[c.rec] = wave_io.pcm_frames(r.path, None, r.utt, channel=channel)[0]
                views.append(maps[c.rec][c.first_sample * r.channels:(c.first_sample + c.samples) * r.channels])
            offs, total = hip.gather_offsets([v.nbytes for v in views], 16)
            off = offs.astype(np.int32)
            samples = np.array([c.samples for c in p], np.int32)
            out_off = np.array([place[c.rec] + c.first_frame for c in p], np.int32)
            pick = channel if r0.channels > 1 else 0
            leg.energy(views, off, samples, out_off, total, r0, remove_dc, pick, max(c.frames for c in p))
            done = [c.rec for c in p if c.first_frame + c.frames == recs[c.rec].frames]
            if done:
                rec_off = np.array([place[i] for i in done], np.int32)
                rec_frames = np.array([recs[i].frames for i in done], np.int32)
                for i, (e, dec) in zip(done, leg.decide(rec_off, rec_frames, opts)):
                    results[i] = (dec, vad.segment(dec, e, *lens))
                    maps.pop(i, None)
        with open(tmp["segments"], "w") as seg, open(tmp["vad.ark"], "wb") as ark, open(tmp["vad.scp"], "w") as scp:
            for i, r in enumerate(recs):
                dec, runs = results.get(i, (np.zeros(0, np.uint8), []))
                entry, at = vector_entry(r.utt, dec.astype(np.float32))
                scp.write("%s %s:%d\n" % (r.utt, final["vad.ark"], ark.tell() + at))
                ark.write(entry)
                if not runs:
                    counters["silent"] += 1
                    print("make_segments: recording %s (%s): no speech found, no segment written" % (r.utt, r.path), file=sys.stderr)
                seg.writelines(segment_lines(r, runs))
                counters["segments"] += len(runs)
        for n in NAMES:
            os.replace(tmp[n], final[n])
    except BaseException:
        for n in NAMES:
            if os.path.exists(tmp[n]):
                os.remove(tmp[n])
        raise
    return dict(counters)


def main(argv=None):
    p = argparse.ArgumentParser(description="a Kaldi segments file from long recordings: an energy VAD (compute-vad-decision's rule) on the device")
    p.add_argument("--data_path", required=True, help="wav.scp: `REC path` lines naming 16-bit WAV recordings (any rate, up to 8 channels)")
    p.add_argument("--out_dir", required=True, help="receives segments, vad.scp and vad.ark")
    p.add_argument("--hip_fbank_conf", default="", help="Kaldi option file of the front end: frame length and shift, --remove-dc-offset, --channel")
    p.add_argument("--vad_conf", default="", help="Kaldi option file of compute-vad-decision: --vad-energy-threshold (5.0), "
                                                  "--vad-energy-mean-scale (0.5), --vad-frames-context (0), --vad-proportion-threshold (0.6)")
    p.add_argument("--min_silence", default=0.3, type=float, help="runs closer than this many seconds are merged")
    p.add_argument("--min_speech", default=0.2, type=float, help="runs shorter than this many seconds are dropped")
    p.add_argument("--pad", default=0.1, type=float, help="seconds added on both ends of a run")
    p.add_argument("--max_segment", default=30.0, type=float, help="a longer run is cut at the first energy minimum of its second half")
    p.add_argument("--chunk_frames", default=60000, type=int, help="frames of one row: a recording is staged in chunks of this many frames")
    p.add_argument("--hip_vad", default="device", choices=["device", "host"],
                   help="device (default): the kernels; host: their serial twins (the comparison leg; needs no GPU)")
    a = p.parse_args(argv)
    c = make_segments(a.data_path, a.out_dir, a.hip_fbank_conf, a.vad_conf, a.min_silence, a.min_speech, a.pad, a.max_segment, a.chunk_frames,
                      a.hip_vad)
    print("make_segments: %d recordings, %d frames in %d passes -> %d segments in %s" % (c["recordings"], c["frames"], c["passes"], c["segments"],
                                                                                       a.out_dir))
    return 0


if __name__ == "__main__":
    sys.exit(main())
