"""FLAC files as a `wav.scp` names them (RFC 9639): which entries are FLAC entries, the metadata chain, and zero-copy access to the
frames with their exact index.

LibriSpeech is distributed as FLAC and the recipe's `local/data_prep.sh` writes every line as `UTT flac -c -d -s /path/UTT.flac |`.
Such an entry - and a plain path to a file that starts with `fLaC` - is read DIRECTLY: no subprocess is ever started.  The file's
bytes travel to the device as they are, about half the bytes of the 16-bit PCM, and are decoded there (``hip.flac_decode``); what the
host contributes is the frame index (``hip.flac_index``: a FLAC frame does not say how long it is), built in one linear pass that
checks every frame's CRC-16 - exact, not a sync-code heuristic.

Only 16-bit streams are read (what the WAV path reads).  Everything else raises a ValueError that names the utterance and the reason.
"""
import mmap
import os
import shlex
from collections import namedtuple

import numpy as np

from .wave_io import _who

# the frames of one file: ``frames`` int32 (n, 3) - byte offset from the first frame, byte length, first sample - and the samples
# per channel they hold
FlacIndex = namedtuple("FlacIndex", "frames samples")
Info = namedtuple("Info", "rate channels bits total audio_offset min_block max_block md5")

_DECODE, _STDOUT, _SILENT = {"-d", "--decode"}, {"-c", "--stdout"}, {"-s", "--silent"}


def _starts_flac(path):
    if not os.path.isfile(path):
        return False
    with open(path, "rb") as f:
        return f.read(4) == b"fLaC"


def command_operand(spec):
    """The file a `flac -c -d -s FILE |` entry names, None when ``spec`` is not that form: token 0 `flac` (or a path to it), then
    exactly one operand and options out of -c -d -s --stdout --decode --silent (short ones may be combined: -cds), decode and stdout
    both present.  Nothing is looked up on disk here."""
    spec = spec.strip()
    if not spec.endswith("|"):
        return None
    try:
        tokens = shlex.split(spec[:-1])
    except ValueError:
        return None
    if len(tokens) < 2 or os.path.basename(tokens[0]) != "flac":
        return None
    seen, operands = set(), []
    for tok in tokens[1:]:
        if tok.startswith("--"):
            if tok not in _DECODE | _STDOUT | _SILENT:
                return None
            seen.add(tok)
        elif tok.startswith("-") and len(tok) > 1:
            if any(ch not in "cds" for ch in tok[1:]):
                return None
            seen.update("-" + ch for ch in tok[1:])
        else:
            operands.append(tok)
    if len(operands) != 1 or not (seen & _DECODE) or not (seen & _STDOUT):
        return None
    return operands[0]


def flac_path(spec):
    """The FLAC file behind an `.scp` entry - a plain path to an existing file that starts with `fLaC`, or the recipe's command form
    naming one - else None."""
    spec = spec.strip()
    path = command_operand(spec) if spec.endswith("|") else spec
    return path if path is not None and _starts_flac(path) else None


def is_flac(spec):
    return flac_path(spec) is not None


def read_info(path, utt=None):
    """STREAMINFO and where the audio starts: `fLaC`, then the metadata blocks walked by their 24-bit lengths up to the last-block
    flag (PADDING, SEEKTABLE, VORBIS_COMMENT, pictures: whatever they hold is skipped, sync patterns included)."""
    who = _who(path, utt)
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(4)
        if head[:3] == b"ID3":
            raise ValueError("%s: the file starts with an ID3 tag, not with `fLaC` (strip the tag: it is not part of a FLAC stream)" % who)
        if head == b"OggS":
            raise ValueError("%s: an Ogg container (Ogg FLAC) is not read, only native FLAC streams" % who)
        if head != b"fLaC":
            raise ValueError("%s: not a FLAC stream (no `fLaC` marker)" % who)
        pos, first, info = 4, True, None
        while True:
            f.seek(pos)
            bh = f.read(4)
            if len(bh) < 4:
                raise ValueError("%s: truncated metadata chain (the file ends at byte %d inside it)" % (who, size))
            last, kind, length = bool(bh[0] & 0x80), bh[0] & 0x7F, int.from_bytes(bh[1:], "big")
            if first:
                body = f.read(34)
                if kind != 0 or length != 34 or len(body) < 34:
                    raise ValueError("%s: the first metadata block is not a STREAMINFO of 34 bytes" % who)
                packed = int.from_bytes(body[10:18], "big")
                info = (packed >> 44, ((packed >> 41) & 7) + 1, ((packed >> 36) & 31) + 1, packed & ((1 << 36) - 1),
                        int.from_bytes(body[0:2], "big"), int.from_bytes(body[2:4], "big"), bytes(body[18:34]))
                first = False
            elif kind == 127:
                raise ValueError("%s: metadata block type 127 is invalid" % who)
            pos += 4 + length
            if pos > size:
                raise ValueError("%s: truncated metadata chain (a block of %d bytes ends behind the file's %d)" % (who, length, size))
            if last:
                break
    rate, channels, bits, total, min_bs, max_bs, md5 = info
    return Info(rate, channels, bits, total, pos, min_bs, max_bs, md5)


def checked(path, sample_rate, utt=None, allow_downsample=False, allow_upsample=False, channel=-1):
    """``read_info`` of a file the front-end admits - the rules of ``wave_io`` for WAV files: 16 bits, the rate the front-end's or
    admitted by --allow-downsample / --allow-upsample, one channel or --channel naming one."""
    info = read_info(path, utt)
    who = _who(path, utt)
    if info.bits != 16:
        raise ValueError("%s: %d-bit samples, only 16-bit FLAC streams are read" % (who, info.bits))
    if info.rate < 1:
        raise ValueError("%s: sample rate %d Hz in STREAMINFO" % (who, info.rate))
    channels, channel = info.channels, int(channel)
    if channels != 1 and not 0 <= channel < channels:
        if channel < 0:
            raise ValueError("%s: %d channels, only one channel is read (--channel=0 .. %d chooses it)" % (who, channels, channels - 1))
        raise ValueError("%s: %d channels, --channel=%d does not name one of them (--channel=0 .. %d)" % (who, channels, channel, channels - 1))
    if sample_rate is not None and info.rate != int(round(float(sample_rate))):
        want = int(round(float(sample_rate)))
        if info.rate > want and not allow_downsample:
            raise ValueError("%s: sample rate %d Hz, the front-end is set to %d Hz (no resampling; --allow-downsample=true admits it)" % (who, info.rate, want))
        if info.rate < want and not allow_upsample:
            raise ValueError("%s: sample rate %d Hz, the front-end is set to %d Hz (no resampling; --allow-upsample=true admits it)" % (who, info.rate, want))
    return info


def audio_view(path, info):
    """A read-only uint8 view of the memory-mapped file from the first audio frame to the end (no copy; the map goes with the view)."""
    n = os.path.getsize(path) - info.audio_offset
    if n <= 0:
        return np.zeros(0, np.uint8)
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    return np.frombuffer(mm, dtype=np.uint8, count=n, offset=info.audio_offset)


def frame_index(path, info, utt=None, view=None):
    """The file's exact frame index (``hip.flac_index``) -> ``FlacIndex``.  Refused, naming the utterance: a stream in which no chain of
    frames with matching CRC-16s reaches the end (with the byte offset where it broke), frames whose rate, channels or sample size
    differ from STREAMINFO's, a total that is not STREAMINFO's (0 there means unknown: the index says it)."""
    from .. import hip

    view = audio_view(path, info) if view is None else view
    who = _who(path, utt)
    if view.shape[0] == 0:
        raise ValueError("%s: no audio frames behind the metadata" % who)
    hint = (info.total // info.min_block + 1) if info.total and info.min_block >= 16 else 0
    try:
        frames, samples = hip.flac_index(view, info.rate, info.channels, info.bits, hint)
    except hip.FlacIndexError as e:
        if e.code == -3:
            raise ValueError("%s: frames whose sample rate, channels or bits differ from STREAMINFO are not read: %s" % (who, e))
        raise ValueError("%s: %s (offsets count from the first frame, byte %d of the file)" % (who, e, info.audio_offset))
    if info.total and samples != info.total:
        raise ValueError("%s: the frames hold %d samples, STREAMINFO says %d" % (who, samples, info.total))
    return FlacIndex(frames, samples)


def num_samples(path, sample_rate=None, utt=None):
    """Samples per channel from the metadata alone - or, for a STREAMINFO total of 0 (unknown), from the index."""
    info = checked(path, sample_rate, utt, True, True, 0)
    return info.total if info.total else frame_index(path, info, utt).samples
