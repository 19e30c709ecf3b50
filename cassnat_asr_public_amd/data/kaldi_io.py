"""Minimal Kaldi table I/O (binary matrices in .ark files addressed by .scp lines): float32 / float64 matrices and the three
compressed kinds.

The reference delegates this to the third-party `kaldiio` package (src/data/speech_loader.py:6,142, pinned 2.15.1 in
requirements_original.txt), which is not available offline.  `kaldiio.load_mat` decompresses transparently, and Kaldi's feature
scripts (`steps/make_fbank.sh`, `copy-feats --compress=true`) write compressed matrices by default, so a real `feats.scp` usually
points into `CM` archives.

Compressed matrices (a restatement of Kaldi's matrix/compressed-matrix.{h,cc}).  At an `.scp` offset the object starts with `\\0B` and
a token:

  * `CM `  is format 1 (3 bytes),
  * `CM2 ` is format 2 (4 bytes),
  * `CM3 ` is format 3 (4 bytes).

Sixteen raw bytes follow - no `\\x04` size prefixes, all little endian: float32 min_value, float32 range, int32 num_rows, int32
num_cols.  Behind them:

  * format 1: num_cols column headers of four uint16 each (p0, p25, p75, p100), then num_cols * num_rows uint8, COLUMN-major:
    byte[c * num_rows + r];
  * format 2: num_rows * num_cols uint16, row-major;
  * format 3: num_rows * num_cols uint8, row-major.

`copy-feats --compress=true` writes `CM` for matrices of more than 8 rows and `CM2` for shorter ones: one archive can hold both
kinds - the kind is a property of the utterance, not of the file.

Decompression is float32 arithmetic, every operation rounded on its own, in the order written (Kaldi's x86 builds use no fused
multiply-add):

    u16(v)   = min_value + (range * 1.52590218966964e-05f) * float(v)      # formats 1 (headers) and 2 (data)
    u8(v)    = min_value + (range * (1/255.0f)) * float(v)                 # format 3
    format 1, column c, P0..P100 = u16(p0..p100 of c), byte b:
      b <= 64 : P0  + ((P25  - P0 ) * float(b      )) * (1/64.0f)
      b <= 192: P25 + ((P75  - P25) * float(b - 64 )) * (1/128.0f)
      else    : P75 + ((P100 - P75) * float(b - 192)) * (1/63.0f)

`decompress` below is that in numpy float32 - the definition the device kernel (csrc/rowops.hip: unpack_compressed_kernel) is held
to bit for bit.  `write_ark_scp(compress=k)` writes valid, tight archives of the three kinds for tests and tools; it does not
reproduce the bytes of Kaldi's own encoder (its quartile indices and its rounding differ).  The writer that follows
`copy-feats --compress=true` - DESIGN.md 7n - is bin/make_fbank: the device kernel cn_op_compress_feats and its host twin;
``matrix_entry`` and ``cmvn_stats_bytes`` below write its archive entries and its statistics file.
"""
import mmap
import os
import struct
import threading

import numpy as np

_DTYPES = {b"FM ": np.float32, b"DM ": np.float64}
# kind of a compressed matrix -> its number in the device kernel's per-utterance metadata (= Kaldi's format number)
COMPRESSED_KINDS = {"CM": 1, "CM2": 2, "CM3": 3}
_HEAD = 22  # the longest header: \0B + "CM2 " + 16 bytes

_U16_INC = np.float32(1.52590218966964e-05)
_U8_INC = np.float32(1) / np.float32(255)
_K64, _K128, _K63 = np.float32(1) / np.float32(64), np.float32(1) / np.float32(128), np.float32(1) / np.float32(63)


def _parse_header(head):
    """The first bytes of a binary matrix object -> (kind, rows, cols, where the payload starts, its bytes).  kind: "FM" / "DM" (the
    payload is the rows) or "CM" / "CM2" / "CM3" (the payload starts at min_value: global header, column headers, data)."""
    head = bytes(head)
    if head[:2] != b"\0B":
        raise ValueError("not a binary Kaldi object")
    tag = head[2:5]
    if tag in _DTYPES:
        if len(head) < 15:
            raise ValueError("truncated Kaldi matrix")
        if head[5:6] != b"\x04" or head[10:11] != b"\x04":
            raise ValueError("corrupt Kaldi matrix header")
        rows, cols = struct.unpack("<i", head[6:10])[0], struct.unpack("<i", head[11:15])[0]
        if rows < 0 or cols < 0:
            raise ValueError("truncated Kaldi matrix")
        return tag[:2].decode(), rows, cols, 15, rows * cols * np.dtype(_DTYPES[tag]).itemsize
    if tag == b"CM ":
        kind, start = "CM", 5
    elif head[2:6] in (b"CM2 ", b"CM3 "):
        kind, start = tag.decode(), 6
    else:
        raise ValueError("unsupported Kaldi matrix type %r" % tag)
    if len(head) < start + 16:
        raise ValueError("truncated Kaldi matrix")
    rows, cols = struct.unpack("<ii", head[start + 8 : start + 16])
    if rows < 0 or cols < 0:
        raise ValueError("truncated Kaldi matrix")
    nbytes = 16 + {"CM": 8 * cols + rows * cols, "CM2": 2 * rows * cols, "CM3": rows * cols}[kind]
    return kind, rows, cols, start, nbytes


def decompress(kind, rows, cols, payload):
    """A compressed matrix's payload (uint8 array starting at min_value) -> the float32 (rows, cols) matrix, in Kaldi's float32
    arithmetic (module docstring): numpy rounds every float32 operation on its own."""
    payload = np.asarray(payload, dtype=np.uint8)
    mn, rng = (np.float32(x) for x in np.frombuffer(payload[:8].tobytes(), "<f4"))
    if kind == "CM2":
        v = np.frombuffer(payload[16 : 16 + 2 * rows * cols].tobytes(), "<u2").astype(np.float32)
        return (mn + (rng * _U16_INC) * v).reshape(rows, cols)
    if kind == "CM3":
        v = payload[16 : 16 + rows * cols].astype(np.float32)
        return (mn + (rng * _U8_INC) * v).reshape(rows, cols)
    if kind != "CM":
        raise ValueError("not a compressed Kaldi matrix kind: %r" % (kind,))
    h = np.frombuffer(payload[16 : 16 + 8 * cols].tobytes(), "<u2").astype(np.float32).reshape(cols, 4)
    p = mn + (rng * _U16_INC) * h
    p0, p25, p75, p100 = (p[:, k : k + 1] for k in range(4))
    b = payload[16 + 8 * cols : 16 + 8 * cols + rows * cols].reshape(cols, rows)
    f = b.astype(np.float32)
    lo = p0 + ((p25 - p0) * f) * _K64
    mid = p25 + ((p75 - p25) * (f - np.float32(64))) * _K128
    hi = p75 + ((p100 - p75) * (f - np.float32(192))) * _K63
    return np.ascontiguousarray(np.where(b <= 64, lo, np.where(b <= 192, mid, hi)).T, dtype=np.float32)


def _read_matrix(f):
    base = f.tell()
    kind, rows, cols, start, nbytes = _parse_header(f.read(_HEAD))
    f.seek(base + start)
    raw = f.read(nbytes)
    if len(raw) != nbytes:
        raise ValueError("truncated Kaldi matrix")
    if kind in COMPRESSED_KINDS:
        return decompress(kind, rows, cols, np.frombuffer(raw, np.uint8))
    dt = np.dtype(_DTYPES[kind.encode() + b" "]).newbyteorder("<")
    return np.frombuffer(raw, dtype=dt).reshape(rows, cols).copy()


def load_mat(rxspecifier):
    """"path" or "path:offset" (an .scp entry) -> numpy matrix (a compressed one decompressed: float32)."""
    path, _, off = rxspecifier.rpartition(":")
    if not path or not off.isdigit():
        path, off = rxspecifier, None
    with open(path, "rb") as f:
        if off is not None:
            f.seek(int(off))
        else:  # a bare file may start with "key "
            head = f.read(2)
            f.seek(0)
            if head != b"\0B":
                while f.read(1) not in (b" ", b""):
                    pass
        return _read_matrix(f)


_maps = {}
_maps_lock = threading.Lock()


def _mapped(path):
    """A read-only memory map of an archive, kept while the file stays the same (a test-set decode reads every matrix of a
    handful of archives once: one map per file instead of one open + seven small reads + a copy per utterance).  The map is
    keyed on the file's identity - inode, size, modification time: an archive rewritten or truncated at the same path gets a new
    map (the stale one stays alive only as long as views into it do)."""
    st = os.stat(path)
    ident = (st.st_ino, st.st_size, st.st_mtime_ns)
    hit = _maps.get(path)
    if hit is None or hit[0] != ident:
        with _maps_lock:
            hit = _maps.get(path)
            if hit is None or hit[0] != ident:
                with open(path, "rb") as f:
                    hit = (ident, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ))
                _maps[path] = hit  # (a replaced map is not closed: numpy views handed out earlier keep it alive)
    return hit[1]


def _entry_header(rxspecifier):
    """(kind, rows, cols) of a "path:offset" entry from its header alone; None for anything else."""
    path, _, off = rxspecifier.rpartition(":")
    if not path or not off.isdigit():
        return None
    with open(path, "rb") as f:
        f.seek(int(off))
        head = f.read(_HEAD)
    try:
        return _parse_header(head)[:3]
    except ValueError as e:
        if "truncated" in str(e):
            raise
        raise ValueError("not a binary Kaldi matrix at %s" % rxspecifier) from None


def mat_dtype(rxspecifier):
    """Element type (numpy dtype) of an .scp entry's matrix, from its header (a compressed matrix reads as float32)."""
    h = _entry_header(rxspecifier)
    if h is None:
        return load_mat(rxspecifier).dtype
    return np.dtype(np.float64 if h[0] == "DM" else np.float32)


def mat_kind(rxspecifier):
    """Kind of an .scp entry's matrix - "FM", "DM", "CM", "CM2" or "CM3" - from its header in the memory map of the archive (no
    open per entry: cheap enough to ask of every utterance of a test set)."""
    path, _, off = rxspecifier.rpartition(":")
    if not path or not off.isdigit():
        return "DM" if load_mat(rxspecifier).dtype == np.float64 else "FM"
    o = int(off)
    return _parse_header(_mapped(path)[o : o + _HEAD])[0]


def mat_payload(rxspecifier):
    """"path:offset" (an .scp entry) -> (kind, rows, cols, payload): what the packed reader stages, nothing decompressed.  kind is
    "FM", "DM", "CM", "CM2" or "CM3"; payload a READ-ONLY uint8 view into the memory map of the archive - for "FM" / "DM" the
    matrix's rows, for a compressed kind everything from min_value on (global header, column headers, data).  Anything else (a
    plain path: one matrix per file) falls back to load_mat, as load_mat_view does: the loaded matrix's own bytes, as "FM" / "DM"
    (a compressed file arrives decompressed: "FM", which is also what mat_kind says of it)."""
    path, _, off = rxspecifier.rpartition(":")
    if not path or not off.isdigit():
        mat = np.ascontiguousarray(load_mat(rxspecifier))
        mat = mat.astype(mat.dtype.newbyteorder("<"), copy=False)
        payload = mat.reshape(-1).view(np.uint8)
        payload.flags.writeable = False
        return ("DM" if mat.dtype == np.float64 else "FM"), mat.shape[0], mat.shape[1], payload
    mm = _mapped(path)
    o = int(off)
    kind, rows, cols, start, nbytes = _parse_header(mm[o : o + _HEAD])
    if o + start + nbytes > len(mm):
        raise ValueError("truncated Kaldi matrix")
    return kind, rows, cols, np.frombuffer(mm, dtype=np.uint8, count=nbytes, offset=o + start)


def load_mat_view(rxspecifier):
    """"path:offset" (an .scp entry) -> a READ-ONLY numpy view of the matrix inside a memory map of the archive (no copy;
    valid as long as the process lives).  A compressed matrix has no in-place form: it comes back decompressed, as a fresh float32
    array.  Anything else falls back to load_mat."""
    path, _, off = rxspecifier.rpartition(":")
    if not path or not off.isdigit():
        return load_mat(rxspecifier)
    kind, rows, cols, payload = mat_payload(rxspecifier)
    if kind in COMPRESSED_KINDS:
        return decompress(kind, rows, cols, payload)
    dt = np.dtype(_DTYPES[kind.encode() + b" "]).newbyteorder("<")
    return payload.view(dt).reshape(rows, cols)


def mat_rows(rxspecifier):
    """Number of rows (frames) of an .scp entry from its header alone - what `feat-to-len` gives."""
    h = _entry_header(rxspecifier)
    if h is None:
        return load_mat(rxspecifier).shape[0]
    return h[1]


def read_scp(scp_path):
    """-> list of (utt, rxspecifier) in file order."""
    out = []
    with open(scp_path, "r") as f:
        for line in f:
            line = line.strip()
            if line:
                utt, spec = line.split(None, 1)
                out.append((utt, spec))
    return out


def _to_u16(v, mn, rng):
    return np.clip(np.floor((v - mn) / rng * 65535.0 + 0.499), 0, 65535).astype("<u2")


def compress_mat(mat, kind):
    """A matrix -> (token, payload bytes) of compressed kind 1 / 2 / 3 (CM / CM2 / CM3): valid and tight, not Kaldi's own bytes.
    The range is the matrix's global [min, max] (max = min + 1 + |min| for a constant matrix); a uint16 is
    floor((v - min) / range * 65535 + 0.499); format 1's column headers are the column's sorted values at indices 0, n/4, 3n/4,
    n-1, forced strictly increasing, and a byte is the nearest code of the segment its value falls in, measured against the
    headers as the reader dequantises them."""
    mat = np.asarray(mat, dtype=np.float64)
    if mat.ndim != 2:
        raise ValueError("compress_mat: a matrix has two axes")
    rows, cols = mat.shape
    lo64, hi64 = (float(mat.min()), float(mat.max())) if mat.size else (0.0, 0.0)
    mn, mx = np.float32(lo64), np.float32(hi64)
    if mn > lo64:  # (a float64 matrix: rounding to float32 must not cut the range short)
        mn = np.nextafter(mn, np.float32(-np.inf))
    if mx < hi64:
        mx = np.nextafter(mx, np.float32(np.inf))
    if mx == mn:
        mx = np.float32(mn + 1 + abs(mn))
    rng = np.float32(mx - mn)
    head = struct.pack("<ffii", mn, rng, rows, cols)
    mn64, rng64 = float(mn), float(rng)
    if kind == 2:
        return b"CM2 ", head + _to_u16(mat, mn64, rng64).tobytes()
    if kind == 3:
        return b"CM3 ", head + np.clip(np.floor((mat - mn64) / rng64 * 255.0 + 0.499), 0, 255).astype(np.uint8).tobytes()
    if kind != 1:
        raise ValueError("compress_mat: kind is 1, 2 or 3, got %r" % (kind,))
    if rows == 0:
        return b"CM ", head + np.zeros((cols, 4), "<u2").tobytes()
    srt = np.sort(mat, axis=0)
    h = _to_u16(srt[[0, rows // 4, 3 * rows // 4, rows - 1]].T, mn64, rng64).astype(np.int64)  # (cols, 4)
    h[:, 0] = np.minimum(h[:, 0], 65532)
    h[:, 1] = np.clip(h[:, 1], h[:, 0] + 1, 65533)
    h[:, 2] = np.clip(h[:, 2], h[:, 1] + 1, 65534)
    h[:, 3] = np.maximum(h[:, 3], h[:, 2] + 1)
    p = (mn + (rng * _U16_INC) * h.astype(np.float32)).astype(np.float64)  # the reader's P0..P100
    p0, p25, p75, p100 = (p[:, k : k + 1] for k in range(4))
    v = mat.T  # (cols, rows): the byte order of the format
    lo = np.clip(np.floor((v - p0) / (p25 - p0) * 64 + 0.5), 0, 64)
    mid = 64 + np.clip(np.floor((v - p25) / (p75 - p25) * 128 + 0.5), 0, 128)
    hi = 192 + np.clip(np.floor((v - p75) / (p100 - p75) * 63 + 0.5), 0, 63)
    b = np.where(v < p25, lo, np.where(v < p75, mid, hi)).astype(np.uint8)
    return b"CM ", head + h.astype("<u2").tobytes() + np.ascontiguousarray(b).tobytes()


def write_ark_scp(ark_path, scp_path, items, compress=None):
    """items: iterable of (utt, matrix).  Writes float32/float64 binary matrices and the matching .scp; with ``compress`` = 1, 2 or
    3 every matrix is written compressed instead (`CM` / `CM2` / `CM3`, see ``compress_mat``)."""
    if compress not in (None, 1, 2, 3):
        raise ValueError("write_ark_scp: compress is None, 1, 2 or 3")
    with open(ark_path, "wb") as ark, open(scp_path, "w") as scp:
        for utt, mat in items:
            mat = np.ascontiguousarray(mat)
            ark.write(utt.encode() + b" ")
            scp.write("%s %s:%d\n" % (utt, ark_path, ark.tell()))
            if compress is not None:
                token, payload = compress_mat(mat, compress)
                ark.write(b"\0B" + token + payload)
                continue
            tag = b"DM " if mat.dtype == np.float64 else b"FM "
            if tag == b"FM ":
                mat = mat.astype("<f4", copy=False)
            ark.write(b"\0B" + tag + b"\x04" + struct.pack("<i", mat.shape[0]) + b"\x04" + struct.pack("<i", mat.shape[1]))
            ark.write(mat.tobytes())


def matrix_entry(utt, mat=None, payload=None):
    """The bytes of one archive entry and the offset of its `\\0B` inside them: ``UTT `` then, for ``mat`` (float32 / float64), the
    `FM ` / `DM ` matrix as ``write_ark_scp`` writes it, or, for ``payload`` (a compressed matrix from min_value on, as
    ``mat_payload`` hands it out and bin/make_fbank's compression writes it), `CM ` / `CM2 ` + the payload - the kind is the one
    `copy-feats --compress=true` chooses: format 1 for more than 8 rows, format 2 otherwise."""
    key = utt.encode() + b" "
    if payload is not None:
        payload = bytes(payload)
        rows, cols = struct.unpack("<ii", payload[8:16])
        token = b"CM " if rows > 8 else b"CM2 "
        if len(payload) != 16 + (8 * cols + rows * cols if rows > 8 else 2 * rows * cols):
            raise ValueError("matrix_entry: %s: a payload of %d bytes for a %d x %d compressed matrix" % (utt, len(payload), rows, cols))
        return key + b"\0B" + token + payload, len(key)
    mat = np.ascontiguousarray(mat)
    tag = b"DM " if mat.dtype == np.float64 else b"FM "
    mat = mat.astype("<f8" if tag == b"DM " else "<f4", copy=False)
    return (key + b"\0B" + tag + b"\x04" + struct.pack("<i", mat.shape[0]) + b"\x04" + struct.pack("<i", mat.shape[1]) + mat.tobytes(), len(key))


def cmvn_stats_bytes(sums, sumsq, count):
    """Kaldi's global CMVN statistics as ``SpeechDataset._load_cmvn`` reads them: a bare `\\0BDM ` matrix of 2 x (F + 1) - the sums and
    the frame count, then the sums of squares and 0."""
    stats = np.zeros((2, len(sums) + 1), "<f8")
    stats[0, :-1], stats[0, -1], stats[1, :-1] = sums, count, sumsq
    return matrix_entry("", stats)[0][1:]
