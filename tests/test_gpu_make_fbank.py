"""bin/make_fbank on the device, end to end, on a handful of synthetic utterances of 0.05 - 2 s: the float32 archive against cn_fbank
bit for bit, the compressed one against the model (tests/feats_model.py) byte for byte, cmvn.ark through the dataset's reader, decode_asr
from the archives against decode_asr from the wav.scp line for line, FLAC / other rates against their WAV twins, the host leg against
the device leg, and a bad file."""
import math
import os

import numpy as np
import pytest

import feats_model as M
from conftest import tiny_case
from test_gpu_flac_reader import channel_conf, rate_set, stereo_set, twin_scps
from test_gpu_spliced_reader import Runs, nat_conf, tiny240
from test_gpu_wave_reader import int16_wave, write_model, write_wav
from test_make_fbank_host import read_dir
from cassnat_asr_public_amd.bin import make_fbank as mf
from cassnat_asr_public_amd.data import kaldi_io
from cassnat_asr_public_amd.data.fbank import Fbank
from cassnat_asr_public_amd.data.speech_loader import SpeechDataset

pytestmark = pytest.mark.gpu

COUNTS = [61, 3, 50, 8, 199, 9, 47]  # frames: 0.05 s (3 frames) to 2 s; 3 and 8 are written as CM2, 9 is the shortest CM
_cache = {}


def wave_of(n, seed):
    """n int16 samples of the reader tests' signal (which lasts 1.2 s: a longer utterance is pieces of it in a row)."""
    return np.concatenate([int16_wave(min(19200, n - at), seed + 50 * k) for k, at in enumerate(range(0, n, 19200))])


def wav_set(tmp_path, counts=COUNTS):
    views, lines = [], []
    for b, n in enumerate(counts):
        x = wave_of(400 + 160 * (n - 1) + (37 * b) % 160, 20 + b)
        views.append(x)
        lines.append("spk-utt%02d %s\n" % (b, write_wav(tmp_path / ("utt%02d.wav" % b), x)))
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    return str(scp), views


def cn_fbank_rows(views, counts):
    """cn_fbank on float32 copies of the samples (computed once, shared)."""
    key = tuple(counts)
    if key not in _cache:
        import torch

        ref, _ = Fbank()([w.astype(np.float32) for w in views])
        torch.cuda.synchronize()
        ref = ref.cpu().numpy()
        _cache[key] = [ref[b, :n].copy() for b, n in enumerate(counts)]
    return _cache[key]


def entries(out):
    return kaldi_io.read_scp(os.path.join(out, "feats.scp"))


def test_the_float32_archive_holds_cn_fbanks_rows(tmp_path):
    scp, views = wav_set(tmp_path)
    out = str(tmp_path / "fm")
    c = mf.make_fbank(scp, out, compress=False, batch_size=3)
    rows = cn_fbank_rows(views, COUNTS)
    table = entries(out)
    assert [u for u, _ in table] == ["spk-utt%02d" % b for b in range(len(COUNTS))] and c["frames"] == sum(COUNTS)
    for (u, spec), want in zip(table, rows):
        assert kaldi_io.mat_kind(spec) == "FM"
        np.testing.assert_array_equal(kaldi_io.load_mat(spec), want)
    assert open(os.path.join(out, "utt2num_frames")).read() == "".join("spk-utt%02d %d\n" % (b, n) for b, n in enumerate(COUNTS))


def test_the_compressed_archive_holds_the_models_bytes(tmp_path):
    scp, views = wav_set(tmp_path)
    out = str(tmp_path / "cm")
    mf.make_fbank(scp, out, batch_size=3)
    rows = cn_fbank_rows(views, COUNTS)
    ark = open(os.path.join(out, "feats.ark"), "rb").read()
    kinds, stored = [], []
    for (u, spec), x in zip(entries(out), rows):
        status, token, payload = M.compress(x)
        at = int(spec.rpartition(":")[2])
        assert status == 0 and ark[at - len(u) - 1:at + 2 + len(token) + len(payload)] == u.encode() + b" \0B" + token + payload, u
        kind = token.decode().strip()
        back = kaldi_io.load_mat(spec)
        np.testing.assert_array_equal(back, kaldi_io.decompress(kind, x.shape[0], x.shape[1], np.frombuffer(payload, np.uint8)))
        kinds.append(kaldi_io.mat_kind(spec))
        stored.append(back)
    assert kinds == ["CM" if n > 8 else "CM2" for n in COUNTS] and {"CM", "CM2"} == set(kinds)
    # cmvn.ark: read by the dataset, and within the bound of any summation order of the values the archive holds
    ds = SpeechDataset.__new__(SpeechDataset)
    ds._load_cmvn(os.path.join(out, "cmvn.ark"))
    stats = kaldi_io.load_mat(os.path.join(out, "cmvn.ark"))
    allv = np.vstack(stored).astype(np.float64)
    assert stats.shape == (2, 81) and stats[0, -1] == sum(COUNTS) and stats[1, -1] == 0
    assert (np.abs(stats[:, :-1] - M.exact_stats(allv)) <= M.stats_bound(allv)).all()
    np.testing.assert_allclose(ds.mean, allv.mean(0), rtol=1e-12, atol=1e-12)
    assert np.isfinite(ds.std).all() and (ds.std > 0).all()


@pytest.mark.parametrize("compress", [True, False])
def test_the_host_leg_writes_the_same_directory(tmp_path, compress):
    scp, _ = wav_set(tmp_path)
    dirs = {}
    for leg in ("device", "host"):
        out = str(tmp_path / "out")  # (the same name: the scp holds the archive's path)
        mf.make_fbank(scp, out, compress=compress, batch_size=3, hip_compress=leg)
        dirs[leg] = read_dir(out)
    assert sorted(dirs["device"]) == sorted(mf.NAMES) and dirs["device"] == dirs["host"]


@pytest.mark.parametrize("files", ["stereo", "rates"])
def test_flac_and_other_rates_give_the_archives_of_their_wav_twins(tmp_path, files):
    counts = [41, 7, 39, 43]
    fscp, wscp = twin_scps(tmp_path, rate_set(counts) if files == "rates" else stereo_set(counts))
    conf = channel_conf(tmp_path, resample=files == "rates")
    dirs = {}
    for name, scp, audio in (("flac", fscp, "flac"), ("wav", wscp, "wav")):
        out = str(tmp_path / "out")
        c = mf.make_fbank(scp, out, fbank_conf=conf, batch_size=3, hip_audio=audio)
        dirs[name] = read_dir(out)
        assert c["frames"] == sum(counts)
    assert dirs["flac"] == dirs["wav"]
    with pytest.raises(ValueError, match="hip_audio"):
        mf.make_fbank(wscp, str(tmp_path / "o2"), fbank_conf=conf, hip_audio="flac")


@pytest.mark.parametrize("right_ctx", [0, 2])
def test_decode_from_the_archives_is_decode_from_the_audio(tmp_path, monkeypatch, right_ctx):
    """decode_asr on the float32 archive with the tool's cmvn.ark writes the result file of decode_asr on the wav.scp with the same
    cmvn.ark, line for line - the pipelined path and the plain loop, unspliced and with right_ctx 2 (the decoder splices) - and the
    compressed archive decodes through the packed reader's compressed form."""
    counts = [61, 37, 50, 44, 58, 39, 47]
    scp, _ = wav_set(tmp_path, counts)
    fm, cm = str(tmp_path / "fm"), str(tmp_path / "cm")
    mf.make_fbank(scp, fm, compress=False, batch_size=4)
    mf.make_fbank(scp, cm, batch_size=4)
    if right_ctx:
        args, state = tiny240()
    else:
        args, state, _, _ = tiny_case()
    cmvn = os.path.join(fm, "cmvn.ark")
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, use_cmvn=True, global_cmvn=cmvn))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    for pipelines in ((1, 2) if not right_ctx else (2,)):
        flags = ["--hip_pipelines", pipelines, "--hip_precision", "fp32"]
        wav, arch = run(scp, *flags), run(os.path.join(fm, "feats.scp"), *flags)
        assert wav == arch and [ln.split()[0] for ln in wav] == ["spk-utt%02d" % b for b in range(len(counts))]
        assert all(len(ln.split()) > 1 for ln in wav)
    n = len(run.stats)
    comp = run(os.path.join(cm, "feats.scp"), "--hip_pipelines", 2, "--hip_precision", "fp32")
    assert len(comp) == len(counts) and run.stats[n]["compressed_passes"] == run.stats[n]["passes"] >= 1, run.stats[n]


def test_a_too_short_file_ends_the_run_and_leaves_no_archive(tmp_path):
    scp, _ = wav_set(tmp_path, [20, 12])
    write_wav(tmp_path / "short.wav", int16_wave(399, 5))  # (one sample short of an analysis window)
    with open(scp, "a") as f:
        f.write("spk-short %s\n" % (tmp_path / "short.wav"))
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="spk-short"):
        mf.make_fbank(scp, out)
    assert not os.path.exists(os.path.join(out, "feats.ark")) and (not os.path.isdir(out) or os.listdir(out) == [])
    # the command line on the set without that file
    good = tmp_path / "good.scp"
    good.write_text("".join(ln for ln in open(scp) if "spk-short" not in ln))
    assert mf.main(["--data_path", str(good), "--out_dir", out, "--batch_size", "2"]) == 0
    assert sorted(os.listdir(out)) == sorted(mf.NAMES) and math.isfinite(kaldi_io.load_mat(os.path.join(out, "cmvn.ark")).sum())
