"""FLAC input on the device, end to end: Fbank.packed and the packed reader's FLAC form against the WAV twins of the same samples -
bit for bit, since FLAC is lossless and everything behind cn_op_flac_decode is the WAV path - decode_asr from a `wav.scp` of FLAC
entries against the one of the WAV twins line for line, and tools/check_flac_files.py on the files the tests' model wrote."""
import io
import os
import sys

import numpy as np
import pytest
import torch

import flac_cases as fc
import flac_model as fm
from conftest import REPO, ast_tiny_case, tiny_case
from test_gpu_spliced_reader import Runs, nat_conf, tiny240
from test_gpu_wave_reader import int16_wave, write_model
from test_gpu_wave_resample import interleave, noise
from test_wave_io_host import fmt_chunk, riff
from cassnat_asr_public_amd.data import flac_io, wave_io
from cassnat_asr_public_amd.data.fbank import Fbank
from cassnat_asr_public_amd.pipeline import DecodePipelines, PackedBatch

pytestmark = pytest.mark.gpu

PAD = -1.5
SIZES = [4096, 1152, 576, 4608, 192, 4097, 2304]
MODES = [1, 10, 8, 9]


def mixed_frames(pcm, k):
    """Frames of block sizes that change from frame to frame (a variable-blocksize stream) and, for two channels, stereo modes that do."""
    pcm = np.asarray(pcm, np.int64).reshape(len(pcm), -1)
    out, at, j = [], 0, k
    while at < len(pcm):
        chunk = pcm[at:at + SIZES[j % len(SIZES)]]
        order = min(2 + j % 3, len(chunk))
        out.append({"pcm": chunk, "assignment": MODES[j % 4] if pcm.shape[1] == 2 else pcm.shape[1] - 1,
                    "subframes": [fm.fixed_sub(order) for _ in range(pcm.shape[1])]})
        at, j = at + len(chunk), j + 1
    return out


def twin(tmp_path, name, pcm, rate=16000, k=0):
    """One FLAC file and the WAV file of the same samples -> (flac path, wav path)."""
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    data = fm.write_stream(mixed_frames(pcm, k), rate=rate, variable=True, blocks=[(1, bytes(k))] if k % 2 else ())[0]
    f = tmp_path / (name + ".flac")
    f.write_bytes(data)
    return str(f), riff(tmp_path / (name + ".wav"), [fmt_chunk(rate=rate, channels=pcm.shape[1])], pcm.astype("<i2").tobytes())


def twin_scps(tmp_path, files):
    """`files`: (pcm, rate) per utterance -> (flac.scp - plain paths and `flac -c -d -s PATH |` in turn -, wav.scp)."""
    fl, wl = [], []
    for b, (pcm, rate) in enumerate(files):
        f, w = twin(tmp_path, "utt%02d" % b, pcm, rate, b)
        fl.append("spk-utt%02d %s\n" % (b, f if b % 2 else "flac -c -d -s %s |" % f))
        wl.append("spk-utt%02d %s\n" % (b, w))
    (tmp_path / "flac.scp").write_text("".join(fl))
    (tmp_path / "wav.scp").write_text("".join(wl))
    return str(tmp_path / "flac.scp"), str(tmp_path / "wav.scp")


def samples_for(n, b):
    return 400 + 160 * (n - 1) + (37 * b) % 160


def stereo_set(counts):
    """Mono and two-channel 16 kHz utterances in turn (channel 1 is read: the conf of ``channel_conf``)."""
    return [(int16_wave(samples_for(n, b), 20 + b) if b % 2 == 0 else interleave(noise(samples_for(n, b), 20 + b), 2, 1, 80 + b).reshape(-1, 2), 16000)
            for b, n in enumerate(counts)]


def rate_set(counts):
    kinds = [(44100, 2), (8000, 1), (16000, 1)]
    out = []
    for b, n in enumerate(counts):
        rate, C = kinds[b % 3]
        out.append((interleave(noise(samples_for(n, b) * rate // 16000, 20 + b), C, min(1, C - 1), 80 + b).reshape(-1, C), rate))
    return out


def channel_conf(tmp_path, resample=False):
    conf = tmp_path / "fbank.conf"
    conf.write_text(("--allow-downsample=true\n--allow-upsample=true\n" if resample else "") + "--channel=1\n")
    return str(conf)


def loaded(path, flac, **admit):
    """What the dataset hands the front-end for one file: (view, rate, channels[, index])."""
    if not flac:
        return wave_io.pcm_frames(path, 16000, None, **admit)
    info = flac_io.checked(path, 16000, None, **admit)
    view = flac_io.audio_view(path, info)
    return view, info.rate, info.channels, flac_io.frame_index(path, info, None, view)


# ------------------------------------------------------------------------------------------------- Fbank.packed
@pytest.mark.parametrize("with_cmvn", [False, True])
@pytest.mark.parametrize("splice", [None, (0, 2, 1)])
@pytest.mark.parametrize("files", ["plain", "rates"])
def test_packed_from_flac_is_packed_from_wav(tmp_path, with_cmvn, splice, files):
    admit = dict(allow_downsample=True, allow_upsample=True, channel=1) if files == "rates" else {}
    sets = rate_set([41, 39, 43]) if files == "rates" else [(int16_wave(n, i), 16000) for i, n in enumerate([400, 559, 6935, 4097])]
    paths = [twin(tmp_path, "u%d" % b, pcm, rate, b) for b, (pcm, rate) in enumerate(sets)]
    rng = np.random.default_rng(3)
    cmvn = dict(cmvn_mean=rng.standard_normal(80) * 3 + 12, cmvn_std=rng.random(80) + 0.5) if with_cmvn else {}
    fb = Fbank(pad_value=PAD, splice=splice, **cmvn, **admit)
    fl = [loaded(f, True, **admit) for f, _ in paths]
    wv = [loaded(w, False, **admit) for _, w in paths]
    assert [x[1:3] for x in fl] == [x[1:3] for x in wv]
    a, ra = fb.packed([x[0] for x in fl], rates=[x[1] for x in fl], channels=[x[2] for x in fl], flac=[x[3] for x in fl])
    b, rb = fb.packed([x[0] for x in wv], rates=[x[1] for x in wv], channels=[x[2] for x in wv])
    torch.cuda.synchronize()
    assert a.shape == b.shape and torch.equal(a, b) and torch.equal(ra, rb) and fb.flac_passes == 1
    assert fb.resampled_passes == (2 if files == "rates" else 0)


# ------------------------------------------------------------------------------------------------- the packed reader
def test_pipelines_stage_a_flac_pass(tmp_path):
    from cassnat_asr_public_amd import synth
    from test_gpu_pipeline import build as build_model

    args = synth.make_args("tiny")
    args.hip_max_batch, args.hip_max_frames = 4, 90
    model = build_model(args, synth.make_state(args, seed=0, gain=2.0), "fp32")
    rng = np.random.default_rng(3)
    cmvn = (rng.standard_normal(80) * 3 + 12, rng.random(80) + 0.5)
    fb = Fbank(cmvn_mean=cmvn[0], cmvn_std=cmvn[1], pad_value=PAD, channel=1)
    sets = stereo_set([41, 39, 43, 42])
    paths = [twin(tmp_path, "u%d" % b, pcm, rate, b) for b, (pcm, rate) in enumerate(sets)]
    fl = [loaded(f, True, channel=1) for f, _ in paths]
    wv = [loaded(w, False, channel=1) for _, w in paths]
    frames = [fb.num_frames(x[3].samples) for x in fl]

    def batch(idx, flac=True):
        src = fl if flac else wv
        return PackedBatch.from_waves([src[i][0] for i in idx], [frames[i] for i in idx], 80, utts=["u%d" % i for i in idx],
                                      formats=[src[i][1:3] for i in idx], channel=1, index=[src[i][3] for i in idx] if flac else None)

    with DecodePipelines(model, 1, 4, 90, cmvn=cmvn, fbank=fb.o) as pipes:
        pipes._on_gpu, pipes._device = True, torch.cuda.current_device()  # (what the first decode() would set: no worker thread here)
        pbs = [batch([0]), batch([1, 2]), batch([3])]
        feats, ratios = pipes._stage_packed(0, 0, [(pb, pb.ratios(), j) for j, pb in enumerate(pbs)], PAD)
        torch.cuda.synchronize()
        pipes._flac_checks[0].pop(0)()  # the status word of the pass: nothing to report
        assert tuple(feats.shape) == (4, 43, 80) and pipes.stats["flac_passes"] == 1 and pipes.stats["wave_passes"] == 1
        assert pipes.stats["resampled_passes"] == 1  # (two channels: the channel pick is the resampler's)
        want, wr = fb.packed([x[0] for x in wv], rates=[x[1] for x in wv], channels=[x[2] for x in wv])
        torch.cuda.synchronize()
        assert torch.equal(feats, want) and len(wr) == 4
        assert torch.equal(ratios.cpu(), torch.cat([pb.ratios() for pb in pbs]))  # (each batch's own ratios, as collate gives them)
        # a second pass reuses the slot's buffers
        bufs = pipes._packed[0][("flac", 0)]
        ptrs = {k: bufs[k].data_ptr() for k in ("host", "dev", "pcm", "fl_scratch", "fl_d")}
        feats2, _ = pipes._stage_packed(0, 0, [(pbs[1], pbs[1].ratios(), 0)], PAD)
        torch.cuda.synchronize()
        pipes._flac_checks[0].pop(0)()
        assert torch.equal(feats2, want[1:3])
        assert {k: pipes._packed[0][("flac", 0)][k].data_ptr() for k in ptrs} == ptrs and pipes.stats["flac_passes"] == 2
        # FLAC batches do not share a pass with WAV batches
        with pytest.raises(ValueError, match="mixes"):
            pipes._stage_packed(0, 1, [(pbs[0], pbs[0].ratios(), 0), (batch([1], flac=False), batch([1], flac=False).ratios(), 1)], PAD)


# ------------------------------------------------------------------------------------------------- decode_asr
COUNTS = [61, 37, 50, 44, 58, 39, 47]


@pytest.mark.parametrize("pipelines", [1, 2])
def test_cassnat_decode_from_a_flac_scp(tmp_path, monkeypatch, pipelines):
    args, state, _, _ = tiny_case()
    fscp, wscp = twin_scps(tmp_path, stereo_set(COUNTS))
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    flags = ["--hip_pipelines", pipelines, "--hip_precision", "fp32", "--hip_fbank_conf", channel_conf(tmp_path)]
    flac, wav = run(fscp, *flags), run(wscp, *flags)
    assert [ln.split()[0] for ln in flac] == ["spk-utt%02d" % b for b in range(len(COUNTS))] and all(len(ln.split()) > 1 for ln in flac)
    assert flac == wav
    s = run.stats
    if pipelines > 1:
        assert s[0]["passes"] >= 1 and s[0]["flac_passes"] == s[0]["wave_passes"] == s[0]["passes"] and s[1]["flac_passes"] == 0, s
    else:
        assert not s[0] and not s[1]
    assert flac == run(fscp, "--hip_audio", "1", *flags)


def test_cassnat_decode_from_a_flac_scp_with_right_ctx_2(tmp_path, monkeypatch):
    args, state = tiny240()
    fscp, wscp = twin_scps(tmp_path, [(int16_wave(samples_for(n, b), 20 + b), 16000) for b, n in enumerate(COUNTS)])
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    flac, wav = run(fscp, "--hip_precision", "fp32"), run(wscp, "--hip_precision", "fp32")
    assert flac == wav and len(flac) == len(COUNTS) and all(len(ln.split()) > 1 for ln in flac)
    assert run.stats[0]["flac_passes"] == run.stats[0]["spliced_passes"] == run.stats[0]["passes"] >= 1 and run.stats[0]["resampled_passes"] == 0


def test_cassnat_ctc_only_from_a_flac_scp(tmp_path, monkeypatch):
    args, state, _, _ = tiny_case()
    fscp, wscp = twin_scps(tmp_path, stereo_set([61, 50, 37, 44]))
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, decode_type="ctc_only", sample_num=1, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    flags = ["--hip_precision", "fp32", "--hip_fbank_conf", channel_conf(tmp_path)]
    flac, wav = run(fscp, *flags), run(wscp, *flags)
    assert flac == wav and len(flac) == 4


def test_art_decode_from_a_flac_scp(tmp_path, monkeypatch):
    args, state, _ = ast_tiny_case(ctc_weight=0.3)
    fscp, wscp = twin_scps(tmp_path, stereo_set([61, 57, 51, 40]))
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight",
                                          "max_decode_ratio", "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(n_features=80, model_type="transformer", beam_width=3, decode_type="ctc_att")
    ckpt, cfg = write_model(tmp_path, args, state, conf)
    run = Runs(tmp_path, monkeypatch, ckpt, cfg, task="art", batch_size=2)
    flags = ["--hip_precision", "fp32", "--hip_fbank_conf", channel_conf(tmp_path)]
    flac, wav = run(fscp, *flags), run(wscp, *flags)
    assert flac == wav and [ln.split()[0] for ln in flac] == ["spk-utt%02d" % b for b in range(4)]


@pytest.mark.parametrize("pipelines", [1, 2])
def test_decode_from_flac_at_other_rates_and_channels(tmp_path, monkeypatch, pipelines):
    args, state, _, _ = tiny_case()
    fscp, wscp = twin_scps(tmp_path, rate_set(COUNTS))
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    flags = ["--hip_pipelines", pipelines, "--hip_precision", "fp32", "--hip_fbank_conf", channel_conf(tmp_path, resample=True)]
    flac, wav = run(fscp, *flags), run(wscp, *flags)
    assert flac == wav and len(flac) == len(COUNTS) and all(len(ln.split()) > 1 for ln in flac)
    if pipelines > 1:
        s = run.stats[0]
        assert s["flac_passes"] == s["resampled_passes"] == s["passes"] >= 1, s


# ------------------------------------------------------------------------------------------------- the tool
def test_check_flac_files_on_the_models_files(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_flac_files

    paths = []
    for u in fc.utterances():
        p = tmp_path / (u["name"] + ".flac")
        p.write_bytes(u["data"])
        paths.append(str(p))
        pcm, info = check_flac_files.decode_file(str(p))
        np.testing.assert_array_equal(pcm, u["pcm"])
    out = io.StringIO()
    assert check_flac_files.check(paths, out) == 0
    lines = out.getvalue().splitlines()
    assert len(lines) == 6 and all(": OK " in ln for ln in lines), lines
    bad = bytearray(fc.utterances()[0]["data"])
    bad[4 + 4 + 20] ^= 1  # a stored signature that is not the PCM's
    (tmp_path / "bad.flac").write_bytes(bytes(bad))
    out = io.StringIO()
    assert check_flac_files.check([str(tmp_path / "bad.flac"), str(tmp_path / "missing.flac")], out) == 2
    assert "MISMATCH" in out.getvalue() and "REFUSED" in out.getvalue()
