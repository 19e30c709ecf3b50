"""Kaldi compressed matrices (`CM`, `CM2`, `CM3`: what `copy-feats --compress=true` and steps/make_fbank.sh write) on the host: the
reader against Kaldi's float32 arithmetic restated here, the encoder's round trip, the dataset / loader over a compressed archive,
the compressed form of pipeline.PackedBatch and the aligned host gather.  No GPU."""
import struct

import numpy as np
import pytest
import torch

from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.data import kaldi_io
from cassnat_asr_public_amd.data.speech_loader import SpeechDataLoader, SpeechDataset
from cassnat_asr_public_amd.data.vocab import Vocab
from cassnat_asr_public_amd.pipeline import PackedBatch

f32 = np.float32
INC16 = f32(1.52590218966964e-05)


def ref_u16(mn, rng, v):
    return f32(mn) + (f32(rng) * INC16) * v.astype(f32)


def ref_u8(mn, rng, v):
    return f32(mn) + (f32(rng) * (f32(1) / f32(255))) * v.astype(f32)


def ref_format1(mn, rng, headers, colbytes):
    """headers (cols, 4) uint16, colbytes (cols, rows) uint8 -> (rows, cols) float32: Kaldi's CharToFloat, one rounding per operation."""
    cols, rows = colbytes.shape
    out = np.empty((rows, cols), f32)
    for c in range(cols):
        p0, p25, p75, p100 = (ref_u16(mn, rng, np.array(h)) for h in headers[c])
        for r in range(rows):
            b = int(colbytes[c, r])
            if b <= 64:
                out[r, c] = p0 + ((p25 - p0) * f32(b)) * (f32(1) / f32(64))
            elif b <= 192:
                out[r, c] = p25 + ((p75 - p25) * f32(b - 64)) * (f32(1) / f32(128))
            else:
                out[r, c] = p75 + ((p100 - p75) * f32(b - 192)) * (f32(1) / f32(63))
    return out


def obj(kind, mn, rng, rows, cols, body):
    token = {1: b"CM ", 2: b"CM2 ", 3: b"CM3 "}[kind]
    return b"\0B" + token + struct.pack("<ffii", f32(mn), f32(rng), rows, cols) + body


def write_objects(tmp_path, objects, name="c"):
    """[(utt, object bytes)] -> (ark path, [rxspecifier])"""
    ark = str(tmp_path / (name + ".ark"))
    specs = []
    with open(ark, "wb") as f:
        for utt, o in objects:
            f.write(utt.encode() + b" ")
            specs.append("%s:%d" % (ark, f.tell()))
            f.write(o)
    return ark, specs


def test_known_answer_of_format_1(tmp_path):
    """A hand-assembled `\\0BCM ` object through load_mat, bit for bit (the bytes hit both ends of every segment)."""
    headers = np.array([[0, 16384, 49152, 65535], [7, 1000, 30000, 65000], [100, 101, 102, 103]], "<u2")
    colbytes = np.array([[0, 64, 65, 192, 193, 255], [1, 63, 128, 191, 200, 254], [0, 64, 65, 192, 193, 255]], np.uint8)
    _, (spec,) = write_objects(tmp_path, [("u", obj(1, -3.25, 21.7, 6, 3, headers.tobytes() + colbytes.tobytes()))])
    want = ("c0500000 c04f85da c04de17e 400b3490 c03b2317 c04ddc11 4010a162 3ff0f196 c04ddc06 "
            "4150676c 40d379b0 c04dd6a4 4151c81e 41027bff c04dd68e 4193999a 4190b610 c04dd137").split()
    for load in (kaldi_io.load_mat, kaldi_io.load_mat_view):
        got = load(spec)
        assert got.dtype == np.float32 and got.shape == (6, 3)
        assert ["%08x" % x for x in np.ascontiguousarray(got).view(np.uint32).ravel()] == want
    np.testing.assert_array_equal(kaldi_io.load_mat(spec), ref_format1(-3.25, 21.7, headers, colbytes))


def test_known_answers_of_formats_2_and_3(tmp_path):
    v16 = np.array([[0, 1, 32767], [32768, 65534, 65535]], "<u2")
    v8 = np.array([[0, 1, 127], [128, 254, 255]], np.uint8)
    _, specs = write_objects(tmp_path, [("a", obj(2, -3.25, 21.7, 2, 3, v16.tobytes())), ("b", obj(3, -3.25, 21.7, 2, 3, v8.tobytes()))])
    for load in (kaldi_io.load_mat, kaldi_io.load_mat_view):
        np.testing.assert_array_equal(load(specs[0]), ref_u16(-3.25, 21.7, v16))
        np.testing.assert_array_equal(load(specs[1]), ref_u8(-3.25, 21.7, v8))
    assert kaldi_io.load_mat(specs[0]).dtype == np.float32 and kaldi_io.load_mat(specs[1]).dtype == np.float32


@pytest.mark.parametrize("cols", [1, 7, 80, 83])
def test_every_byte_and_uint16_value_decodes_as_kaldi_does(tmp_path, cols):
    """Random headers and random bytes (not encoder output): all 256 byte values in format 1, the whole uint16 range in format 2,
    all bytes in format 3, against the float32 restatement above."""
    rng = np.random.default_rng(100 + cols)
    objects, want = [], []
    for rows in (1, 2, 8, 9, 33):
        mn, rg = f32(rng.standard_normal() * 5), f32(rng.random() * 40 + 0.1)
        headers = np.sort(rng.integers(0, 65536, size=(cols, 4)), axis=1).astype("<u2")
        colbytes = rng.integers(0, 256, size=(cols, rows)).astype(np.uint8)
        objects.append(("f1r%d" % rows, obj(1, mn, rg, rows, cols, headers.tobytes() + colbytes.tobytes())))
        want.append(ref_format1(mn, rg, headers, colbytes))
        v16 = rng.integers(0, 65536, size=(rows, cols)).astype("<u2")
        objects.append(("f2r%d" % rows, obj(2, mn, rg, rows, cols, v16.tobytes())))
        want.append(ref_u16(mn, rg, v16))
        v8 = rng.integers(0, 256, size=(rows, cols)).astype(np.uint8)
        objects.append(("f3r%d" % rows, obj(3, mn, rg, rows, cols, v8.tobytes())))
        want.append(ref_u8(mn, rg, v8))
    # every byte value in one format 1 column set, and every uint16 in one format 2 matrix
    headers = np.sort(rng.integers(0, 65536, size=(cols, 4)), axis=1).astype("<u2")
    colbytes = np.stack([rng.permutation(256) for _ in range(cols)]).astype(np.uint8)
    objects.append(("allbytes", obj(1, -7.5, 30.25, 256, cols, headers.tobytes() + colbytes.tobytes())))
    want.append(ref_format1(-7.5, 30.25, headers, colbytes))
    n16 = -(-65536 // cols)
    v16 = (np.arange(n16 * cols) % 65536).astype("<u2").reshape(n16, cols)
    objects.append(("allu16", obj(2, -7.5, 30.25, n16, cols, v16.tobytes())))
    want.append(ref_u16(-7.5, 30.25, v16))
    _, specs = write_objects(tmp_path, objects)
    for spec, w in zip(specs, want):
        np.testing.assert_array_equal(kaldi_io.load_mat(spec), w)
        np.testing.assert_array_equal(kaldi_io.load_mat_view(spec), w)


def _bound(kind, spec, cols):
    """Per column: one quantisation step of the entry as written."""
    _, rows, _, payload = kaldi_io.mat_payload(spec)
    mn, rg = (float(x) for x in np.frombuffer(payload[:8].tobytes(), "<f4"))
    if kind == 2:
        return np.full(cols, rg / 65535)
    if kind == 3:
        return np.full(cols, rg / 255)
    p = mn + rg / 65535 * np.frombuffer(payload[16 : 16 + 8 * cols].tobytes(), "<u2").reshape(cols, 4).astype(np.float64)
    return np.maximum.reduce([(p[:, 1] - p[:, 0]) / 64, (p[:, 2] - p[:, 1]) / 128, (p[:, 3] - p[:, 2]) / 63]) + rg / 65535


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_write_then_read_is_within_one_quantisation_step(tmp_path, kind):
    """write_ark_scp(compress=k) -> load_mat on N(0.5, 3^2) matrices: |error| <= range/65535 (format 2), range/255 (format 3), the
    column's largest segment step + range/65535 (format 1); a constant matrix (max == min) comes back exactly."""
    rng = np.random.default_rng(kind)
    mats = [("n%d_f%d" % (n, F), (rng.standard_normal((n, F)) * 3 + 0.5).astype(np.float32)) for n in (1, 3, 61, 200) for F in (7, 80)]
    mats.append(("const", np.full((5, 4), -2.5, np.float32)))
    scp = str(tmp_path / "r.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "r.ark"), scp, mats, compress=kind)
    entries = kaldi_io.read_scp(scp)
    assert [u for u, _ in entries] == [u for u, _ in mats]
    token = {1: b"CM ", 2: b"CM2 ", 3: b"CM3 "}[kind]
    raw = open(str(tmp_path / "r.ark"), "rb").read()
    for (utt, spec), (_, m) in zip(entries, mats):
        o = int(spec.rpartition(":")[2])
        assert raw[o : o + 2 + len(token)] == b"\0B" + token and raw[o - len(utt) - 1 : o] == utt.encode() + b" "
        got = kaldi_io.load_mat(spec)
        assert got.dtype == np.float32 and got.shape == m.shape
        err = np.abs(got.astype(np.float64) - m)
        assert (err <= _bound(kind, spec, m.shape[1])[None]).all(), (utt, err.max())
        if utt == "const":
            np.testing.assert_array_equal(got, m)
    with pytest.raises(ValueError):
        kaldi_io.write_ark_scp(str(tmp_path / "x.ark"), str(tmp_path / "x.scp"), mats[:1], compress=4)


def _mixed_archive(tmp_path, mats, name="m"):
    """One archive as `copy-feats --compress=true` writes it: `CM` for more than 8 rows, `CM2` for shorter matrices."""
    objects = []
    for utt, m in mats:
        token, payload = kaldi_io.compress_mat(m, 1 if m.shape[0] > 8 else 2)
        objects.append((utt, b"\0B" + token + payload))
    ark, specs = write_objects(tmp_path, objects, name)
    scp = str(tmp_path / (name + ".scp"))
    with open(scp, "w") as f:
        f.write("".join("%s %s\n" % (u, s) for (u, _), s in zip(mats, specs)))
    return scp


def test_reader_functions_on_compressed_entries(tmp_path):
    """mat_rows / mat_dtype / mat_kind / mat_payload and read_scp offsets; one archive holding a `CM` and a `CM2` entry; a truncated
    payload and a negative dimension raise."""
    rng = np.random.default_rng(9)
    mats = [("long", (rng.standard_normal((33, 7)) * 3 + 0.5).astype(np.float32)), ("short", (rng.standard_normal((5, 7)) * 3 + 0.5).astype(np.float32))]
    scp = _mixed_archive(tmp_path, mats)
    entries = kaldi_io.read_scp(scp)
    assert [kaldi_io.mat_kind(s) for _, s in entries] == ["CM", "CM2"]
    for (utt, spec), (_, m) in zip(entries, mats):
        assert kaldi_io.mat_rows(spec) == m.shape[0] and kaldi_io.mat_dtype(spec) == np.float32
        kind, rows, cols, payload = kaldi_io.mat_payload(spec)
        assert (rows, cols) == m.shape and payload.dtype == np.uint8 and not payload.flags.writeable
        assert payload.nbytes == 16 + (8 * cols + rows * cols if kind == "CM" else 2 * rows * cols)
        assert struct.unpack("<ii", payload[8:16].tobytes()) == m.shape  # the view starts at min_value
        np.testing.assert_array_equal(kaldi_io.decompress(kind, rows, cols, payload), kaldi_io.load_mat(spec))
        assert np.abs(kaldi_io.load_mat(spec) - m).max() < 0.2
    # a float32 entry: the payload is its rows
    fscp = str(tmp_path / "f.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "f.ark"), fscp, mats[:1])
    kind, rows, cols, payload = kaldi_io.mat_payload(kaldi_io.read_scp(fscp)[0][1])
    assert kind == "FM" and payload.dtype == np.uint8 and not payload.flags.writeable
    np.testing.assert_array_equal(payload.view("<f4").reshape(rows, cols), mats[0][1])
    # truncated: the archive ends inside the payload
    whole = open(str(tmp_path / "m.ark"), "rb").read()
    cut = str(tmp_path / "cut.ark")
    open(cut, "wb").write(whole[:-3])
    last = "%s:%s" % (cut, entries[1][1].rpartition(":")[2])
    for fn in (kaldi_io.load_mat, kaldi_io.load_mat_view, kaldi_io.mat_payload):
        with pytest.raises(ValueError, match="truncated Kaldi matrix"):
            fn(last)
    # negative dimensions
    _, specs = write_objects(tmp_path, [("a", obj(1, 0.0, 1.0, -1, 3, b"")), ("b", obj(3, 0.0, 1.0, 2, -3, b"")), ("c", obj(2, 0.0, 1.0, -2, -2, b""))], "neg")
    for spec in specs:
        for fn in (kaldi_io.load_mat, kaldi_io.load_mat_view, kaldi_io.mat_rows, kaldi_io.mat_payload):
            with pytest.raises(ValueError, match="truncated Kaldi matrix"):
                fn(spec)


def _vocab_file(tmp_path):
    p = tmp_path / "vocab.txt"
    p.write_text("a\nb\nc 7\nutt a b d\n")
    return str(p)


@pytest.mark.parametrize("use_cmvn", [False, True])
@pytest.mark.parametrize("general", [False, True])
def test_dataset_and_loader_over_a_compressed_archive(tmp_path, use_cmvn, general):
    """SpeechDataset + SpeechDataLoader over a compressed archive (`CM` and `CM2` mixed) hand over the tensors of the `FM ` archive
    that holds the decompressed values - with and without the global CMVN; `general`: right_ctx 2 / skip_frame 2, the path
    with splicing and frame skipping."""
    rng = np.random.default_rng(12)
    mats = [("utt%02d" % b, (rng.standard_normal((n, 6)) * 3 + 0.5).astype(np.float32)) for b, n in enumerate([9, 5, 70, 33, 4, 1])]
    cscp = _mixed_archive(tmp_path, mats, "c")
    values = [(u, kaldi_io.load_mat(s)) for u, s in kaldi_io.read_scp(cscp)]
    fscp = str(tmp_path / "f.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "f.ark"), fscp, values)
    allf = np.vstack([m for _, m in values]).astype(np.float64)
    stats = np.zeros((2, 7))
    stats[0, :6], stats[0, 6], stats[1, :6] = allf.sum(0), len(allf), (allf ** 2).sum(0)
    kaldi_io.write_ark_scp(str(tmp_path / "cmvn.ark"), str(tmp_path / "cmvn.scp"), [("global", stats)])
    args = synth.make_args("tiny", left_ctx=0, right_ctx=2 if general else 0, skip_frame=2 if general else 1)
    got = {}
    for name, scp in (("c", cscp), ("f", fscp)):
        ds = SpeechDataset(Vocab(_vocab_file(tmp_path), 1), [{"name": "test", "scp_path": scp}], args)
        if use_cmvn:
            ds._load_cmvn(kaldi_io.read_scp(str(tmp_path / "cmvn.scp"))[0][1])
        assert ds.can_defer_cmvn() == (not general)
        assert ds.matrix_kinds() == ({"CM", "CM2"} if name == "c" else {"FM"})
        got[name] = [(u, f.clone(), r.clone()) for u, f, _, r, _ in SpeechDataLoader(ds, 4, padding_idx=0)]
    assert len(got["c"]) == 2
    for (uc, fc, rc), (uf, ff, rf) in zip(got["c"], got["f"]):
        assert uc == uf and fc.dtype == torch.float32 and torch.equal(fc, ff) and torch.equal(rc, rf)


def test_packed_batch_in_compressed_form(tmp_path):
    """PackedBatch.from_payloads on compressed entries: shape, ratios() and padded() are those of the float32 form over the
    decompressed values (with and without CMVN); a view of another column count, or of the other family, raises and names the
    utterance."""
    rng = np.random.default_rng(13)
    mats = [("u%d" % b, (rng.standard_normal((n, 7)) * 3 + 0.5).astype(np.float32)) for b, n in enumerate([61, 1, 33, 8, 9])]
    cscp = _mixed_archive(tmp_path, mats, "c")
    specs = [s for _, s in kaldi_io.read_scp(cscp)]
    utts = [u for u, _ in mats]
    pc = PackedBatch.from_payloads([kaldi_io.mat_payload(s) for s in specs], utts=utts)
    pf = PackedBatch([kaldi_io.load_mat_view(s) for s in specs])
    assert pc.kinds == [1, 2, 1, 2, 1] and pf.kinds is None
    assert pc.shape == pf.shape == (5, 61, 7) and pc.lens == pf.lens and torch.equal(pc.ratios(), pf.ratios())
    mean, std = rng.standard_normal(7), rng.random(7) + 0.5
    assert torch.equal(pc.padded(0.0), pf.padded(0.0)) and torch.equal(pc.padded(-1.0, (mean, std)), pf.padded(-1.0, (mean, std)))
    # float32 entries through the same door give the float32 form
    fscp = str(tmp_path / "f.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "f.ark"), fscp, mats)
    fspecs = [s for _, s in kaldi_io.read_scp(fscp)]
    pff = PackedBatch.from_payloads([kaldi_io.mat_payload(s) for s in fspecs], utts=utts)
    assert pff.kinds is None and pff.shape == (5, 61, 7) and torch.equal(pff.padded(0.0), PackedBatch([m for _, m in mats]).padded(0.0))
    # contradictions
    other = [("wide", (rng.standard_normal((12, 8)) * 3).astype(np.float32))]
    wscp = _mixed_archive(tmp_path, other, "w")
    wide = kaldi_io.mat_payload(kaldi_io.read_scp(wscp)[0][1])
    entries = [kaldi_io.mat_payload(s) for s in specs[:2]]
    with pytest.raises(ValueError, match="wide"):
        PackedBatch.from_payloads(entries + [wide], utts=["u0", "u1", "wide"])
    with pytest.raises(ValueError, match="u1"):
        PackedBatch.from_payloads([kaldi_io.mat_payload(fspecs[0]), entries[1]], utts=["u0", "u1"])
    with pytest.raises(ValueError, match="u0"):
        PackedBatch.from_payloads(entries, utts=["u0", "u1"], compressed=False)
    with pytest.raises(ValueError, match="u0"):
        PackedBatch.from_payloads(entries, utts=["u0", "u1"], cols=80)
    kind, rows, cols, payload = entries[0]
    with pytest.raises(ValueError, match="u0"):  # a payload that is not the size its header gives
        PackedBatch.from_payloads([(kind, rows, cols, payload[:-1])], utts=["u0"])


def test_host_gather_with_alignment(tmp_path):
    """hip.host_gather(align=16): every piece at the next multiple of 16 bytes, at the returned offsets; the default call packs
    back to back as before."""
    rng = np.random.default_rng(14)
    pieces = [rng.integers(0, 256, size=int(n)).astype(np.uint8) for n in [1, 16, 17, 31, 32, 100, 5, 48]]
    for threads in (1, 3):
        dst = np.full(1024, 0xEE, np.uint8)
        offs = hip.host_gather(dst.ctypes.data, pieces, threads, align=16)
        want, o = [], 0
        for p in pieces:
            want.append(o)
            o += -(-p.size // 16) * 16
        assert offs.tolist() == want
        for p, o in zip(pieces, offs.tolist()):
            np.testing.assert_array_equal(dst[o : o + p.size], p)
            assert (dst[o + p.size : -(-(o + p.size) // 16) * 16] == 0xEE).all()  # the gaps are not written
        assert (dst[int(offs[-1]) + pieces[-1].size :] == 0xEE).all()
    assert hip.gather_offsets([p.size for p in pieces], 16)[1] == want[-1] + pieces[-1].size
    dst = np.full(1024, 0xEE, np.uint8)
    offs = hip.host_gather(dst.ctypes.data, pieces, 2)
    assert offs.tolist() == np.concatenate([[0], np.cumsum([p.size for p in pieces])[:-1]]).tolist()
    np.testing.assert_array_equal(dst[: sum(p.size for p in pieces)], np.concatenate(pieces))
    assert hip.host_gather(dst.ctypes.data, [], 2, align=16).size == 0


def test_plain_path_entries_without_an_offset(tmp_path):
    """An .scp whose entries are plain paths (one binary matrix per file, no `:offset`): every reader function falls back to
    load_mat, mat_payload included - the float32 packed reader takes such a set as before - and a compressed file reads as its
    decompressed float32 values."""
    rng = np.random.default_rng(15)
    mats = [("u%d" % b, (rng.standard_normal((n, 6)) * 3 + 0.5).astype(np.float32)) for b, n in enumerate([9, 5, 33])]
    scp = str(tmp_path / "plain.scp")
    with open(scp, "w") as f:
        for b, (utt, m) in enumerate(mats):
            one = str(tmp_path / (utt + ".ark"))
            kaldi_io.write_ark_scp(one, str(tmp_path / "unused.scp"), [(utt, m)], compress=1 if b == 2 else None)
            f.write("%s %s\n" % (utt, one))
    entries = kaldi_io.read_scp(scp)
    assert all(":" not in spec for _, spec in entries)
    values = [kaldi_io.load_mat(spec) for _, spec in entries]
    np.testing.assert_array_equal(values[0], mats[0][1])
    assert np.abs(values[2] - mats[2][1]).max() < 0.2 and values[2].dtype == np.float32
    for (_, spec), v in zip(entries, values):
        assert kaldi_io.mat_kind(spec) == "FM" and kaldi_io.mat_rows(spec) == v.shape[0] and kaldi_io.mat_dtype(spec) == np.float32
        kind, rows, cols, payload = kaldi_io.mat_payload(spec)
        assert kind == "FM" and (rows, cols) == v.shape and payload.dtype == np.uint8 and not payload.flags.writeable
        np.testing.assert_array_equal(payload.view("<f4").reshape(rows, cols), v)
        np.testing.assert_array_equal(kaldi_io.load_mat_view(spec), v)
    d64 = str(tmp_path / "d.ark")
    kaldi_io.write_ark_scp(d64, str(tmp_path / "unused.scp"), [("d", mats[0][1].astype(np.float64))])
    assert kaldi_io.mat_kind(d64) == "DM" and kaldi_io.mat_payload(d64)[0] == "DM" and kaldi_io.mat_payload(d64)[3].nbytes == 9 * 6 * 8
    # the dataset classifies the set as float32 throughout, and the packed reader's batch is the collated one
    ds = SpeechDataset(Vocab(_vocab_file(tmp_path), 1), [{"name": "test", "scp_path": scp}], synth.make_args("tiny", left_ctx=0, right_ctx=0, skip_frame=1))
    assert ds.can_defer_cmvn() and ds.matrix_kinds() == {"FM"}
    pb = PackedBatch.from_payloads([kaldi_io.mat_payload(spec) for _, spec in entries], utts=[u for u, _ in entries], compressed=False, cols=6)
    _, feats, _, ratios, _ = next(iter(SpeechDataLoader(ds, 3, padding_idx=0)))
    assert pb.kinds is None and pb.shape == tuple(feats.shape) and torch.equal(pb.ratios(), ratios) and torch.equal(pb.padded(0.0), feats)
