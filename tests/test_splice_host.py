"""Frame splicing and skipping in the packed reader, host side: a ``PackedBatch`` with a splice triple is, bit for bit, what
``SpeechDataLoader`` yields through the dataset's general host path (CMVN in float64, zero rows up to a multiple of skip,
``feat_op.context_feat`` / ``skip_feat``, collate's padding) - its ``padded()`` is the definition the device kernel
(``hip.splice_rows``) is held to -, the dataset's predicates, wave sets that splice, and the front-end / model agreement check."""
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cassnat_asr_public_amd.data import kaldi_io
from cassnat_asr_public_amd.data.speech_loader import (SpeechDataLoader, SpeechDataset, WaveBatch, splice_host, splice_triple,
                                                       spliced_frames)
from cassnat_asr_public_amd.pipeline import DecodePipelines, PackedBatch

TRIPLES = [(0, 2, 1), (1, 1, 2), (3, 0, 1), (0, 0, 3), (2, 2, 3)]
LENGTHS = [1, 2, 5, 33, 64, 7]  # T = 1, T % skip != 0 for skip 2 and 3, T % skip == 0 (64 / 2, 33 / 3)
F0 = 12
PAD = -1


def data_args(left, right, skip, **kw):
    a = SimpleNamespace(left_ctx=left, right_ctx=right, skip_frame=skip, rank=1, hip_audio="auto", hip_fbank_conf="")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def matrices(seed=3, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return [("utt%d" % b, (rng.standard_normal((n, F0)) * 2.5 + 4.0).astype(dtype)) for b, n in enumerate(LENGTHS)]


def archive(tmp_path, form, mats=None):
    """The matrices as an `FM ` archive, or a compressed one that mixes `CM` and `CM2` (two archives behind one table)."""
    mats = mats or matrices()
    scp = str(tmp_path / ("%s.scp" % form))
    if form == "fm":
        kaldi_io.write_ark_scp(str(tmp_path / "fm.ark"), scp, mats)
    else:
        kaldi_io.write_ark_scp(str(tmp_path / "c1.ark"), str(tmp_path / "c1.scp"), mats[0::2], compress=1)
        kaldi_io.write_ark_scp(str(tmp_path / "c2.ark"), str(tmp_path / "c2.scp"), mats[1::2], compress=2)
        lines = dict(ln.split(None, 1) for f in ("c1.scp", "c2.scp") for ln in open(str(tmp_path / f)))
        with open(scp, "w") as f:
            f.write("".join("%s %s" % (u, lines[u]) for u, _ in mats))
    return [{"name": "test", "scp_path": scp}]


def cmvn_file(tmp_path):
    rng = np.random.default_rng(8)
    n = 1000.0
    mean, std = rng.standard_normal(F0) * 3 + 12, rng.random(F0) + 0.5  # a mean far from 0: a zero row normalised by mistake shows
    stats = np.zeros((2, F0 + 1))
    stats[0, :-1], stats[0, -1], stats[1, :-1] = mean * n, n, (std ** 2 + mean ** 2) * n
    kaldi_io.write_ark_scp(str(tmp_path / "cmvn.ark"), str(tmp_path / "cmvn.scp"), [("global", stats)])
    return kaldi_io.read_scp(str(tmp_path / "cmvn.scp"))[0][1]


@pytest.mark.parametrize("with_cmvn", [False, True])
@pytest.mark.parametrize("form", ["fm", "compressed"])
@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "%d-%d-%d" % t)
def test_packed_batch_is_the_general_host_path(tmp_path, triple, form, with_cmvn):
    ds = SpeechDataset(None, archive(tmp_path, form), data_args(*triple))
    if with_cmvn:
        ds._load_cmvn(cmvn_file(tmp_path))
    assert ds.device_splice() == triple and ds.splice() == triple and not ds.can_defer_cmvn()
    loader = SpeechDataLoader(ds, 4, padding_idx=PAD)
    blocks = triple[0] + triple[1] + 1
    for idx, (utts, feats, _, ratios, _) in zip(loader.batch_sampler, loader):
        items = [ds._items[i] for i in idx]
        pb = PackedBatch.from_payloads([kaldi_io.mat_payload(spec) for _, spec, _ in items], utts=[u for u, _, _ in items],
                                       compressed=(form != "fm"), cols=F0, splice=triple)
        assert pb.utts == utts and pb.splice == triple
        assert pb.lens == [LENGTHS[i] for i in idx]  # source rows
        assert pb.out_lens == [-(-LENGTHS[i] // triple[2]) for i in idx]
        assert pb.source_shape == (len(idx), max(pb.lens), F0)
        assert pb.shape == tuple(feats.shape) == (len(idx), max(pb.out_lens), blocks * F0)
        assert torch.equal(pb.ratios(), ratios)
        got = pb.padded(PAD, (ds.mean, ds.std) if with_cmvn else None)
        assert got.dtype == torch.float32 and torch.equal(got, feats)
        if triple in ((1, 1, 2), (2, 2, 3)) and with_cmvn:
            # the appended rows are zeros AFTER the CMVN (not (0 - mean) / std), and the right edge replicates them: the newest
            # block of the last kept row of an utterance whose length is no multiple of skip is literal zeros
            for b, i in enumerate(idx):
                if LENGTHS[i] % triple[2]:
                    assert (got[b, pb.out_lens[b] - 1, -F0:] == 0).all()


def test_the_cpu_rehearsal_stages_spliced_batches(tmp_path):
    """DecodePipelines without a GPU hands the engine the collated tensors themselves: a spliced pass of two batches."""
    triple = (0, 2, 1)
    ds = SpeechDataset(None, archive(tmp_path, "fm"), data_args(*triple))
    loader = SpeechDataLoader(ds, 3, padding_idx=PAD)
    pbs, want = [], []
    for idx, (_, feats, _, _, _) in zip(loader.batch_sampler, loader):
        pbs.append(PackedBatch.from_payloads([kaldi_io.mat_payload(ds._items[i][1]) for i in idx], splice=triple))
        want.append(feats)
    pipes = DecodePipelines.__new__(DecodePipelines)
    pipes._on_gpu, pipes._device, pipes.cmvn = False, None, None
    feats, ratios = pipes._stage_packed(0, 0, [(pb, pb.ratios(), j) for j, pb in enumerate(pbs)], float(PAD))
    assert feats.shape == (6, 64, 3 * F0)
    assert torch.equal(feats[:3, :5], want[0]) and (feats[:3, 5:] == PAD).all() and torch.equal(feats[3:], want[1])
    mixed = PackedBatch.from_payloads([kaldi_io.mat_payload(ds._items[0][1])], splice=(0, 1, 1))
    with pytest.raises(ValueError, match="splice"):
        pipes._stage_packed(0, 0, [(pbs[0], pbs[0].ratios(), 0), (mixed, mixed.ratios(), 1)], float(PAD))


def test_helpers():
    assert splice_triple(0, 0, 1) is None and splice_triple(0, 0, 0) is None and splice_triple(0, 2, 1) == (0, 2, 1)
    assert splice_triple(0, 0, 3) == (0, 0, 3)
    assert [spliced_frames(n, (1, 1, 3)) for n in (1, 3, 4, 6)] == [1, 1, 2, 2] and spliced_frames(7, (0, 2, 1)) == 7
    assert spliced_frames(7, None) == 7
    x = np.arange(10, dtype=np.float32).reshape(5, 2)
    got = splice_host(x, (1, 1, 2))  # 5 rows -> 6 with a zero row; rows 0, 2, 4 of the spliced matrix
    np.testing.assert_array_equal(got, [[0, 1, 0, 1, 2, 3], [2, 3, 4, 5, 6, 7], [6, 7, 8, 9, 0, 0]])
    unspliced = PackedBatch([x])
    assert unspliced.splice is None and unspliced.shape == unspliced.source_shape == (1, 5, 2) and unspliced.out_lens == [5]


def test_predicates_for_sets_the_packed_reader_does_not_take(tmp_path):
    dm = str(tmp_path / "dm.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "dm.ark"), dm, matrices(dtype=np.float64))
    ds = SpeechDataset(None, [{"name": "t", "scp_path": dm}], data_args(0, 2, 1))
    assert ds.splice() == (0, 2, 1) and ds.device_splice() is None and not ds.can_defer_cmvn()
    ds = SpeechDataset(None, [{"name": "t", "scp_path": dm}], data_args(0, 0, 1))
    assert ds.splice() is None and ds.device_splice() is None and not ds.can_defer_cmvn()  # (a `DM` archive never defers)
    # a table that mixes the float32 and the compressed family
    fm, cm = archive(tmp_path, "fm")[0]["scp_path"], archive(tmp_path, "compressed")[0]["scp_path"]
    both = tmp_path / "both.scp"
    both.write_text("".join(open(fm).readlines()[:3] + open(cm).readlines()[3:]))
    ds = SpeechDataset(None, [{"name": "t", "scp_path": str(both)}], data_args(0, 2, 1))
    assert ds.matrix_kinds() == {"FM", "CM", "CM2"} and ds.device_splice() is None and not ds.can_defer_cmvn()
    ds = SpeechDataset(None, [{"name": "t", "scp_path": str(both)}], data_args(0, 0, 1))
    assert ds.device_splice() is None and ds.can_defer_cmvn()  # (unspliced: unchanged - the collated path defers the CMVN)
    for form in ("fm", "compressed"):
        ds = SpeechDataset(None, archive(tmp_path, form), data_args(0, 0, 1))
        assert ds.device_splice() is None and ds.can_defer_cmvn()
        ds = SpeechDataset(None, archive(tmp_path, form), data_args(0, 0, 2))
        assert ds.device_splice() == (0, 0, 2) and not ds.can_defer_cmvn()


# ------------------------------------------------------------------------------------------------- audio input
def write_wav(path, n, seed=0):
    x = (np.random.default_rng(seed).standard_normal(n) * 3000).astype("<i2")
    data = x.tobytes()
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + struct.pack("<HHIIHH", 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


def wave_paths(tmp_path, counts):
    p = tmp_path / "wav.scp"
    p.write_text("".join("u%d %s\n" % (i, write_wav(tmp_path / ("u%d.wav" % i), n, i)) for i, n in enumerate(counts)))
    return [{"name": "test", "scp_path": str(p)}]


@pytest.mark.parametrize("right,skip", [(2, 1), (0, 2), (2, 2)])
def test_wave_sets_splice_and_skip(tmp_path, right, skip):
    counts = [400, 559, 560, 6935, 1040]  # 1, 1, 2, 41, 5 frames
    ds = SpeechDataset(None, wave_paths(tmp_path, counts), data_args(0, right, skip))
    triple = (0, right, skip)
    assert ds.is_wave and ds.wave_frames == [1, 1, 2, 41, 5]  # the front-end's own counts
    assert ds.splice() == triple and ds.device_splice() == triple and ds.can_defer_cmvn()
    loader = SpeechDataLoader(ds, 5, padding_idx=0)
    _, feats, _, ratios, _ = next(iter(loader))
    n_out = [-(-n // skip) for n in ds.wave_frames]
    assert isinstance(feats, WaveBatch) and feats.frames == ds.wave_frames and feats.splice == triple
    assert feats.shape == (5, max(n_out), (right + 1) * 80)
    assert torch.equal(ratios, torch.tensor([n / max(n_out) for n in n_out], dtype=torch.float32))
    pb = PackedBatch.from_waves(feats.views, ds.wave_frames, 80, splice=triple)
    assert pb.shape == feats.shape and pb.lens == ds.wave_frames and pb.source_shape == (5, 41, 80) and torch.equal(pb.ratios(), ratios)
    with pytest.raises(NotImplementedError):
        pb.padded()


def test_a_left_context_on_audio_is_still_refused(tmp_path):
    with pytest.raises(NotImplementedError, match="left_ctx") as e:
        SpeechDataset(None, wave_paths(tmp_path, [1600]), data_args(1, 2, 1))
    assert "right_ctx" in str(e.value)  # (the message says what IS taken)


class _Vocab:
    word2index = {"blank": 0, "sos": 1, "eos": 2, "unk": 3}
    n_words = 4


@pytest.mark.parametrize("n_features,input_size,right,skip,ok", [
    (80, 240, 2, 1, True),     # the recipes' decode YAMLs
    (80, 80, 0, 1, True),
    (80, 80, 2, 1, False),     # input_size disagrees with (left + right + 1) // skip * n_features
    (80, 160, 2, 1, False),
    (240, 240, 2, 1, False),   # the reference's formula holds for no front-end: 3 x 80 mel bins are 240, but 3 x 240 are not
    (80, 240, 0, 1, False),
    (80, 160, 1, 2, False),    # 2 // 2 x 80 = 80, not 160
])
def test_front_end_and_model_must_agree_on_the_spliced_width(tmp_path, n_features, input_size, right, skip, ok):
    from cassnat_asr_public_amd.tasks.base_task import BaseTask

    task = BaseTask.__new__(BaseTask)
    task.vocab = _Vocab
    args = data_args(0, right, skip, test_paths=wave_paths(tmp_path, [1600, 3200]), n_features=n_features, input_size=input_size, batch_size=2,
                     padding_idx=0, load_data_workers=0)
    if ok:
        task.set_test_dataloader(args)
        assert task.test_loader.dataset.splice() == splice_triple(0, right, skip)
        return
    with pytest.raises(ValueError, match="80 mel bins.*%d / %d" % (n_features, input_size)):
        task.set_test_dataloader(args)
