"""RIFF/WAVE files as a `wav.scp` names them: header parsing and zero-copy access to the samples.

The reference never opens a sound file - its recipes run Kaldi's `compute-fbank-feats` first - so this is the part of Kaldi's
`wave-reader.cc` the recogniser needs to start from audio: 16-bit PCM; one channel at the front-end's sample rate, or - with the
front-end's `--allow-downsample` / `--allow-upsample` / `--channel` (``wave_format``, ``pcm_frames``) - another rate and several
interleaved channels, of which one is read.  The chunks of
the file are walked (anything may sit before `data`: `LIST`, `fact`, ...; an odd-sized chunk is followed by a pad byte),
`WAVE_FORMAT_EXTENSIBLE` is accepted with the PCM sub-format, and a `data` size of 0 or 0xFFFFFFFF means "to the end of the file", as
Kaldi reads streamed files.  Everything else raises a ValueError that names the utterance and the reason; an `.scp` entry that is a
command (`... |`) or carries a `:offset` is refused too - no subprocess is ever started (the one command form that is taken,
`flac -c -d -s FILE |` on a FLAC stream, is read directly: ``data.flac_io``).

``pcm_view`` hands out a read-only '<i2' view of the samples inside a memory map of the file.  The map lives exactly as long as
the view: nothing is cached here (a test set is thousands of files), the reader drops the views of a pass once it is staged.
"""
import mmap
import os
import struct

import numpy as np

PCM, IEEE_FLOAT, EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
_TO_END = (0, 0xFFFFFFFF)


def _who(path, utt=None):
    return "utterance %s (%s)" % (utt, path) if utt is not None else str(path)


def check_spec(spec, utt=None):
    """An `.scp` entry of a wave set must be a plain path: a command or a `:offset` raises."""
    spec = spec.strip()
    if spec.endswith("|"):
        from . import flac_io

        if flac_io.is_flac(spec):  # (the recipe's `flac -c -d -s FILE |` on a FLAC stream: the file is read directly)
            return spec
        raise ValueError("%s: the entry is a command (ends in '|'): piped wav.scp entries are not read, no subprocess is started "
                         "(only `flac -c -d -s FILE |` is taken, by reading FILE directly, when FILE is a FLAC stream)" % _who(spec, utt))
    path, _, off = spec.rpartition(":")
    if path and off.isdigit():
        raise ValueError("%s: the entry carries a :offset, a wave set names whole files" % _who(spec, utt))
    return spec


def is_wav(spec):
    """A plain path whose first bytes are `RIFF....WAVE` (a Kaldi matrix file starts with `\\0B`, an archive with a key)."""
    spec = spec.strip()
    if spec.endswith("|") or not os.path.isfile(spec):
        return False
    with open(spec, "rb") as f:
        head = f.read(12)
    return len(head) == 12 and head[:4] == b"RIFF" and head[8:12] == b"WAVE"


def read_header(path, utt=None):
    """-> (sample_rate, channels, bits, fmt_tag, data_offset, data_bytes).  ``fmt_tag`` is the format that describes the samples:
    for WAVE_FORMAT_EXTENSIBLE the sub-format's (1 PCM, 3 IEEE float)."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError("%s: not a RIFF/WAVE file" % _who(path, utt))
        fmt = None
        pos = 12
        while True:
            f.seek(pos)
            ck = f.read(8)
            if len(ck) < 8:
                raise ValueError("%s: no %s chunk" % (_who(path, utt), "data" if fmt else "fmt"))
            cid, csize = ck[:4], struct.unpack("<I", ck[4:])[0]
            if cid == b"fmt ":
                body = f.read(min(csize, 40))
                if csize < 16 or len(body) < 16:
                    raise ValueError("%s: truncated fmt chunk" % _who(path, utt))
                tag, channels, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == EXTENSIBLE:
                    if len(body) < 40:
                        raise ValueError("%s: WAVE_FORMAT_EXTENSIBLE without its sub-format" % _who(path, utt))
                    tag = struct.unpack("<H", body[24:26])[0]
                fmt = (rate, channels, bits, tag)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError("%s: data chunk before fmt" % _who(path, utt))
                start = pos + 8
                if csize in _TO_END:
                    csize = size - start
                elif start + csize > size:
                    raise ValueError("%s: the data chunk says %d bytes, the file holds %d behind its header"
                                     % (_who(path, utt), csize, max(0, size - start)))
                return fmt + (start, csize)
            pos += 8 + csize + (csize & 1)


def _checked(path, sample_rate, utt, allow_downsample=False, allow_upsample=False, channel=-1):
    """-> (data offset, samples per channel, rate, channels) of a file the front-end admits; everything else raises, naming the
    utterance and - where there is one - the option that would admit the file."""
    rate, channels, bits, tag, start, nbytes = read_header(path, utt)
    who = _who(path, utt)
    if tag != PCM:
        raise ValueError("%s: format tag %d (%s), only 16-bit PCM is read" % (who, tag, "IEEE float" if tag == IEEE_FLOAT else "not PCM"))
    if bits != 16:
        raise ValueError("%s: %d-bit samples, only 16-bit PCM is read" % (who, bits))
    if channels < 1:
        raise ValueError("%s: %d channels" % (who, channels))
    if channels != 1 and not 0 <= int(channel) < channels:
        if int(channel) < 0:
            raise ValueError("%s: %d channels, only one channel is read (--channel=0 .. %d chooses it)" % (who, channels, channels - 1))
        raise ValueError("%s: %d channels, --channel=%d does not name one of them (--channel=0 .. %d)" % (who, channels, int(channel), channels - 1))
    if sample_rate is not None and int(rate) != int(round(float(sample_rate))):
        want = int(round(float(sample_rate)))
        if rate < 1:
            raise ValueError("%s: sample rate %d Hz" % (who, rate))
        if rate > want and not allow_downsample:
            raise ValueError("%s: sample rate %d Hz, the front-end is set to %d Hz (no resampling; --allow-downsample=true admits it)" % (who, rate, want))
        if rate < want and not allow_upsample:
            raise ValueError("%s: sample rate %d Hz, the front-end is set to %d Hz (no resampling; --allow-upsample=true admits it)" % (who, rate, want))
    return start, nbytes // (2 * channels), int(rate), int(channels)


def num_samples(path, sample_rate=None, utt=None):
    """Samples of the file, from its header alone (checked as ``pcm_view`` checks it)."""
    return _checked(path, sample_rate, utt)[1]


def pcm_view(path, sample_rate=None, utt=None):
    """A read-only '<i2' numpy view of the samples inside a memory map of the file (no copy; the descriptor is closed once the
    file is mapped, the map goes with the last view into it)."""
    return _view(path, *_checked(path, sample_rate, utt)[:2])


def _view(path, start, n):
    if n == 0:
        return np.zeros(0, "<i2")
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    return np.frombuffer(mm, dtype="<i2", count=n, offset=start)


def wave_format(path, sample_rate=None, utt=None, allow_downsample=False, allow_upsample=False, channel=-1):
    """-> (samples per channel, rate, channels) from the header alone, for a front-end with Kaldi's `--allow-downsample`,
    `--allow-upsample` and `--channel` (compute-fbank-feats): a file at a higher rate than ``sample_rate`` needs ``allow_downsample``,
    one at a lower rate ``allow_upsample``, a file of C > 1 channels ``channel`` in [0, C).  ``channel`` = -1 with C > 1 raises: Kaldi
    warns and takes channel 0, here the choice has to be spelled out.  At the defaults this admits what ``pcm_view`` admits."""
    return _checked(path, sample_rate, utt, allow_downsample, allow_upsample, channel)[1:]


def pcm_frames(path, sample_rate=None, utt=None, allow_downsample=False, allow_upsample=False, channel=-1):
    """``pcm_view`` for such a front-end: -> (view, rate, channels), the view the read-only '<i2' INTERLEAVED data chunk (sample j of
    channel c at j * channels + c; whole sample frames only) inside a memory map of the file.  Picking the channel and resampling
    happen on the device (``hip.wave_resample``)."""
    start, n, rate, channels = _checked(path, sample_rate, utt, allow_downsample, allow_upsample, channel)
    return _view(path, start, n * channels), rate, channels
