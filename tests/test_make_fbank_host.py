"""bin/make_fbank without a GPU: the host leg (--hip_compress host) with precomputed float32 rows in place of the device's features
(``make_fbank(rows_of=...)``) - feats.ark, feats.scp, utt2num_frames and cmvn.ark byte for byte against files written here by hand
from the model (tests/feats_model.py), the scp order under a shuffled batch order, temporaries and the rename on failure."""
import os
import struct

import numpy as np
import pytest

import feats_model as M
from cassnat_asr_public_amd.bin import make_fbank as mf
from cassnat_asr_public_amd.data import kaldi_io
from cassnat_asr_public_amd.data.speech_loader import SpeechDataset

UTTS = ["spk-b", "spk-a", "spk-e", "spk-c", "spk-d"]
ROWS = [12, 5, 40, 8, 9]
F = 7


def matrices(seed=3):
    rng = np.random.default_rng(seed)
    return {u: (rng.standard_normal((n, F)) * 2.5 + 0.7).astype(np.float32) for u, n in zip(UTTS, ROWS)}


def names_scp(tmp_path):
    scp = tmp_path / "wav.scp"
    scp.write_text("".join("%s /nowhere/%s.wav\n" % (u, u) for u in UTTS))
    return str(scp)


def by_hand(out_dir, mats, batches, compress):
    """The four files' bytes, written out here: entries in the batches' order, tables in the input order."""
    ark, offsets, total = b"", {}, np.zeros((2, F))
    for batch in batches:
        for i in batch:
            u, x = UTTS[i], mats[UTTS[i]]
            ark += u.encode() + b" "
            offsets[u] = len(ark)
            if compress:
                status, token, payload = M.compress(x)
                assert status == 0
                ark += b"\0B" + token + payload
            else:
                ark += b"\0BFM \x04" + struct.pack("<i", x.shape[0]) + b"\x04" + struct.pack("<i", F) + x.astype("<f4").tobytes()
    for u in UTTS:  # (input order)
        x = mats[u]
        stored = kaldi_io.decompress("CM" if x.shape[0] > 8 else "CM2", x.shape[0], F, np.frombuffer(M.compress(x)[2], np.uint8)) if compress else x
        total += M.stats(stored)
    scp = "".join("%s %s:%d\n" % (u, os.path.join(out_dir, "feats.ark"), offsets[u]) for u in UTTS)
    frames = "".join("%s %d\n" % (u, n) for u, n in zip(UTTS, ROWS))
    cmvn = b"\0BDM \x04" + struct.pack("<i", 2) + b"\x04" + struct.pack("<i", F + 1)
    cmvn += struct.pack("<%dd" % (F + 1), *total[0], float(sum(ROWS))) + struct.pack("<%dd" % (F + 1), *total[1], 0.0)
    return {"feats.ark": ark, "feats.scp": scp.encode(), "utt2num_frames": frames.encode(), "cmvn.ark": cmvn}


def read_dir(out_dir):
    return {n: open(os.path.join(out_dir, n), "rb").read() for n in sorted(os.listdir(out_dir))}


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("order", ["input", "sorted", [[3, 0], [2], [1, 4]]], ids=["input", "sorted", "shuffled"])
def test_the_four_files_byte_for_byte(tmp_path, compress, order):
    mats = matrices()
    out = str(tmp_path / "fbank")
    c = mf.make_fbank(names_scp(tmp_path), out, compress=compress, batch_size=2, hip_compress="host", order=order, rows_of=lambda us: [mats[u] for u in us])
    batches = {"input": [[0, 1], [2, 3], [4]], "sorted": [[0, 1], [2, 3], [4]]}.get(order if isinstance(order, str) else "", order)
    want = by_hand(out, mats, batches, compress)
    got = read_dir(out)
    assert sorted(got) == sorted(want)  # (no temporary is left)
    for n in want:
        assert got[n] == want[n], n
    assert c["utterances"] == 5 and c["frames"] == sum(ROWS) and c["passes"] == 3
    # the scp follows the input, whatever order the entries were written in; every reader of this project reads them
    table = kaldi_io.read_scp(os.path.join(out, "feats.scp"))
    assert [u for u, _ in table] == UTTS
    for (u, spec), n in zip(table, ROWS):
        assert kaldi_io.mat_kind(spec) == (("CM" if n > 8 else "CM2") if compress else "FM") and kaldi_io.mat_rows(spec) == n
        x = mats[u]
        stored = kaldi_io.decompress("CM" if n > 8 else "CM2", n, F, np.frombuffer(M.compress(x)[2], np.uint8)) if compress else x
        np.testing.assert_array_equal(kaldi_io.load_mat(spec), stored)


def test_the_statistics_file_is_what_the_dataset_reads(tmp_path):
    mats = matrices()
    out = str(tmp_path / "fbank")
    mf.make_fbank(names_scp(tmp_path), out, compress=True, batch_size=3, hip_compress="host", rows_of=lambda us: [mats[u] for u in us])
    ds = SpeechDataset.__new__(SpeechDataset)
    ds._load_cmvn(os.path.join(out, "cmvn.ark"))
    stored = np.vstack([kaldi_io.load_mat(spec) for _, spec in kaldi_io.read_scp(os.path.join(out, "feats.scp"))]).astype(np.float64)
    np.testing.assert_allclose(ds.mean, stored.mean(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ds.std, stored.std(0), rtol=1e-9)
    # "sorted" and a shuffled order give the same statistics file: the host adds the utterances in input order
    again = str(tmp_path / "again")
    mf.make_fbank(names_scp(tmp_path), again, compress=True, batch_size=2, hip_compress="host", order=[[4], [1, 0], [3, 2]],
                  rows_of=lambda us: [mats[u] for u in us])
    assert read_dir(out)["cmvn.ark"] == read_dir(again)["cmvn.ark"] and read_dir(out)["utt2num_frames"] == read_dir(again)["utt2num_frames"]


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("bad", ["nan", "empty"])
def test_a_failure_names_the_utterance_and_leaves_nothing_behind(tmp_path, compress, bad):
    mats = matrices()
    mats["spk-c"] = mats["spk-c"].copy()
    if bad == "nan":
        mats["spk-c"][3, 2] = np.nan
    else:
        mats["spk-c"] = np.zeros((0, F), np.float32)
    out = str(tmp_path / "fbank")
    seen = []

    def rows_of(us):
        seen.append(sorted(os.listdir(out)))  # (what lies in the directory while the run is under way)
        return [mats[u] for u in us]

    with pytest.raises(ValueError, match="spk-c"):
        mf.make_fbank(names_scp(tmp_path), out, compress=compress, batch_size=2, hip_compress="host", order="input", rows_of=rows_of)
    assert os.listdir(out) == []
    assert all(not set(mf.NAMES) & set(names) for names in seen) and any(names for names in seen)  # temporaries only, never the final names


def test_a_failed_run_leaves_an_earlier_directory_as_it_was(tmp_path):
    mats = matrices()
    out = str(tmp_path / "fbank")
    mf.make_fbank(names_scp(tmp_path), out, batch_size=2, hip_compress="host", rows_of=lambda us: [mats[u] for u in us])
    before = read_dir(out)
    worse = dict(mats, **{"spk-d": np.full((9, F), np.inf, np.float32)})
    with pytest.raises(ValueError, match="spk-d"):
        mf.make_fbank(names_scp(tmp_path), out, batch_size=2, hip_compress="host", rows_of=lambda us: [worse[u] for u in us])
    assert read_dir(out) == before


def test_refusals(tmp_path):
    mats = matrices()
    with pytest.raises(ValueError, match="host leg"):
        mf.make_fbank(names_scp(tmp_path), str(tmp_path / "o"), hip_compress="device", rows_of=lambda us: [mats[u] for u in us])
    twice = tmp_path / "twice.scp"
    twice.write_text("a /x.wav\na /y.wav\n")
    with pytest.raises(ValueError, match="twice"):
        mf.make_fbank(str(twice), str(tmp_path / "o"), hip_compress="host", rows_of=lambda us: [mats["spk-a"] for _ in us])
    with pytest.raises(SystemExit):
        mf.main(["--data_path", str(twice), "--out_dir", str(tmp_path / "o"), "--compress", "maybe"])
    with pytest.raises(SystemExit):
        mf.main(["--data_path", str(twice), "--out_dir", str(tmp_path / "o"), "--hip_compress", "somewhere"])
    assert not os.path.exists(str(tmp_path / "o")) or os.listdir(str(tmp_path / "o")) == []


def test_archive_entries_written_by_the_added_kaldi_io_functions(tmp_path):
    x = matrices()["spk-b"]
    entry, at = kaldi_io.matrix_entry("u1", mat=x)
    ark = tmp_path / "a.ark"
    kaldi_io.write_ark_scp(str(ark), str(tmp_path / "a.scp"), [("u1", x)])
    assert ark.read_bytes() == entry and at == 3  # (the existing writer's bytes)
    _, token, payload = M.compress(x)
    entry, at = kaldi_io.matrix_entry("u1", payload=payload)
    assert entry == b"u1 \0B" + token + payload and at == 3
    with pytest.raises(ValueError, match="u1"):
        kaldi_io.matrix_entry("u1", payload=payload[:-1])
