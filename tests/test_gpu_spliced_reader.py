"""The recipes' feature configuration (left_ctx 0, right_ctx 2, skip_frame 1: input_size 240 from 80 mel bins) end to end: decode_asr
through the packed reader - float32 archive, compressed archive, wav.scp; CMVN, splice and skip on the device (cn_op_splice_rows) -
against the dataset's host path and the plain loop, line for line; frame skipping with lengths that are no multiple of skip; and
the engine itself at input_size 240 (F1 = 120, F2 = 60, a linear_out K of 60 x d_model) against the oracle."""
import numpy as np
import pytest
import torch

from conftest import ast_tiny_case
from oracle import cassnat_oracle as orc
from test_gpu_pipeline import LOGIT_TOL, build, decode, maxerr
from test_gpu_wave_reader import NAT_KEYS, cmvn_stats, int16_wave, write_model, write_wav
from cassnat_asr_public_amd import synth
from cassnat_asr_public_amd.data import kaldi_io
from cassnat_asr_public_amd.data.fbank import Fbank
from cassnat_asr_public_amd.data.speech_loader import splice_host

pytestmark = pytest.mark.gpu

COUNTS = [61, 37, 50, 44, 58, 39, 47]  # seven utterances, batch size 3: three batches, the last of one utterance


def tiny240(**ov):
    """The tiny model reading spliced frames: 3 x 80 = 240 values (seeded as the tiny case is)."""
    args = synth.make_args("tiny", **dict(dict(input_size=240, n_features=80, right_ctx=2), **ov))
    return args, synth.make_state(args, seed=0, gain=2.0)


def feature_mats(counts, dim=80, seed=5):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, dim)) * 2.5 + 0.7).astype(np.float32) for n in counts]


def fm_archive(tmp_path, mats, name="feats"):
    scp = str(tmp_path / (name + ".scp"))
    kaldi_io.write_ark_scp(str(tmp_path / (name + ".ark")), scp, [("spk-utt%02d" % b, m) for b, m in enumerate(mats)])
    return scp


def mixed_compressed_archive(tmp_path, mats):
    """`CM` and `CM2` entries behind one table, and the `FM ` archive of the values they decompress to."""
    named = [("spk-utt%02d" % b, m) for b, m in enumerate(mats)]
    kaldi_io.write_ark_scp(str(tmp_path / "c1.ark"), str(tmp_path / "c1.scp"), named[0::2], compress=1)
    kaldi_io.write_ark_scp(str(tmp_path / "c2.ark"), str(tmp_path / "c2.scp"), named[1::2], compress=2)
    lines = dict(ln.split(None, 1) for f in ("c1.scp", "c2.scp") for ln in open(str(tmp_path / f)))
    cscp = str(tmp_path / "c.scp")
    with open(cscp, "w") as f:
        f.write("".join("%s %s" % (u, lines[u]) for u, _ in named))
    assert {kaldi_io.mat_kind(s) for _, s in kaldi_io.read_scp(cscp)} == {"CM", "CM2"}
    values = [kaldi_io.load_mat(s) for _, s in kaldi_io.read_scp(cscp)]
    return cscp, fm_archive(tmp_path, values, "twin"), values


def wave_twins(tmp_path, counts, **fbank_opts):
    """WAV files of the given frame counts and the `FM ` archive of the (unspliced) features the device computes from them."""
    views, lines = [], []
    for b, n in enumerate(counts):
        x = int16_wave(400 + 160 * (n - 1) + (37 * b) % 160, 20 + b)
        views.append(x)
        lines.append("spk-utt%02d %s\n" % (b, write_wav(tmp_path / ("utt%02d.wav" % b), x)))
    wscp = tmp_path / "wav.scp"
    wscp.write_text("".join(lines))
    feats, ratios = Fbank(**fbank_opts).packed(views)
    torch.cuda.synchronize()
    feats = feats.cpu().numpy()
    assert [round(float(r) * feats.shape[1]) for r in ratios] == list(counts)
    mats = [feats[b, :n].copy() for b, n in enumerate(counts)]
    return str(wscp), fm_archive(tmp_path, mats), mats


class Runs:
    """decode_asr.main on one model, one call per result file; the pipeline statistics of every call are kept."""

    def __init__(self, tmp_path, monkeypatch, ckpt, cfg, task="cassnat", batch_size=3):
        from cassnat_asr_public_amd.tasks import CassNATTask

        self.tmp_path, self.ckpt, self.cfg, self.task, self.batch_size, self.stats, self.n = tmp_path, ckpt, cfg, task, batch_size, [], 0
        orig, stats = CassNATTask.decode, self.stats

        def decode_(task_, a):
            task_.pipeline_stats = None
            rc = orig(task_, a)
            stats.append(dict(getattr(task_, "pipeline_stats", None) or {}))
            return rc

        monkeypatch.setattr(CassNATTask, "decode", decode_)

    def __call__(self, scp, *flags):
        from cassnat_asr_public_amd.bin import decode_asr

        self.n += 1
        result = str(self.tmp_path / ("res%d.txt" % self.n))
        argv = ["--task", self.task, "--test_config", self.cfg, "--data_path", scp, "--resume_model", self.ckpt, "--result_file", result,
                "--batch_size", str(self.batch_size), "--load_data_workers", "0"] + [str(f) for f in flags]
        assert decode_asr.main(argv) == 0
        return open(result).read().splitlines()


def nat_conf(args, tmp_path=None, mats=None, dim=80, **more):
    conf = {k: getattr(args, k) for k in NAT_KEYS}
    if mats is not None:
        conf.update(use_cmvn=True, global_cmvn=cmvn_stats(tmp_path, mats, dim))
    conf.update(more)
    return conf


# ------------------------------------------------------------------------------------------------- 1. float32 archive
@pytest.mark.parametrize("with_cmvn,precision", [(False, "fp32"), (True, "fp32"), (False, None), (True, None)])
def test_fm_archive_packed_against_host_and_plain(tmp_path, monkeypatch, with_cmvn, precision):
    args, state = tiny240()
    mats = feature_mats(COUNTS)
    scp = fm_archive(tmp_path, mats)
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, tmp_path, mats if with_cmvn else None))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    prec = ["--hip_precision", precision] if precision else []
    packed = run(scp, "--hip_pipelines", 2, *prec)
    host = run(scp, "--hip_pipelines", 2, "--hip_packed_reader", 0, *prec)
    plain = run(scp, "--hip_pipelines", 1, *prec)
    assert [ln.split()[0] for ln in packed] == ["spk-utt%02d" % b for b in range(len(COUNTS))] and all(len(ln.split()) > 1 for ln in packed)
    assert packed == host == plain
    s = run.stats
    assert s[0]["passes"] >= 1 and s[0]["spliced_passes"] == s[0]["passes"] and s[0]["compressed_passes"] == 0, s
    assert s[1]["passes"] >= 1 and s[1]["spliced_passes"] == 0, s
    assert not s[2], s
    if with_cmvn and precision == "fp32":  # --hip_device_cmvn 0 chooses the host path too
        assert run(scp, "--hip_pipelines", 2, "--hip_device_cmvn", 0, *prec) == packed and run.stats[3]["spliced_passes"] == 0


# ------------------------------------------------------------------------------------------------- 2. compressed archive
def test_mixed_compressed_archive_packed_against_host(tmp_path, monkeypatch):
    args, state = tiny240()
    cscp, fscp, values = mixed_compressed_archive(tmp_path, feature_mats(COUNTS))
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, tmp_path, values))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    packed = run(cscp, "--hip_precision", "fp32")
    host = run(cscp, "--hip_precision", "fp32", "--hip_packed_reader", 0)
    twin = run(fscp, "--hip_precision", "fp32")
    assert packed == host == twin and len(packed) == len(COUNTS)
    s = run.stats
    assert s[0]["passes"] >= 1 and s[0]["spliced_passes"] == s[0]["compressed_passes"] == s[0]["passes"], s
    assert s[1]["spliced_passes"] == 0 and s[1]["compressed_passes"] == 0 and s[1]["passes"] >= 1, s
    assert s[2]["spliced_passes"] == s[2]["passes"] and s[2]["compressed_passes"] == 0, s


# ------------------------------------------------------------------------------------------------- 3. wav.scp
@pytest.mark.parametrize("with_cmvn,pipelines,precision", [(False, 2, "fp32"), (True, 2, None), (True, 1, "fp32"), (False, 1, None)])
def test_cassnat_from_a_wav_scp_with_right_ctx_2(tmp_path, monkeypatch, with_cmvn, pipelines, precision):
    args, state = tiny240()
    wscp, fscp, mats = wave_twins(tmp_path, COUNTS)
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, tmp_path, mats if with_cmvn else None))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    flags = ["--hip_pipelines", pipelines] + (["--hip_precision", precision] if precision else [])
    wav, fm = run(wscp, *flags), run(fscp, *flags)
    assert [ln.split()[0] for ln in wav] == ["spk-utt%02d" % b for b in range(len(COUNTS))]
    assert wav == fm
    s = run.stats
    if pipelines > 1:
        assert s[0]["passes"] >= 1 and s[0]["wave_passes"] == s[0]["spliced_passes"] == s[0]["passes"], s
        assert s[1]["wave_passes"] == 0 and s[1]["spliced_passes"] == s[1]["passes"], s
    else:
        assert not s[0] and not s[1]


def test_ctc_only_from_a_wav_scp_with_right_ctx_2(tmp_path, monkeypatch):
    """decode_type ctc_only keeps the plain loop: BaseTask.wave_features splices the audio batch (Fbank.packed)."""
    args, state = tiny240()
    wscp, fscp, _ = wave_twins(tmp_path, [61, 50, 37, 44])
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, decode_type="ctc_only", sample_num=1, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2,
                                                            ctc_lm_weight=0))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    wav, fm = run(wscp, "--hip_precision", "fp32"), run(fscp, "--hip_precision", "fp32")
    assert wav == fm and len(wav) == 4


def test_art_ctc_att_from_a_wav_scp_with_right_ctx_2(tmp_path, monkeypatch):
    """ArtTask, ctc_att beam 3: its workers splice the audio batches on their own streams."""
    args, state, _ = ast_tiny_case(ctc_weight=0.3, input_size=240)
    wscp, fscp, _ = wave_twins(tmp_path, [61, 57, 51, 40])
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight",
                                          "max_decode_ratio", "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(n_features=80, right_ctx=2, model_type="transformer", beam_width=3, decode_type="ctc_att")
    ckpt, cfg = write_model(tmp_path, args, state, conf)
    run = Runs(tmp_path, monkeypatch, ckpt, cfg, task="art", batch_size=2)
    wav, fm = run(wscp, "--hip_precision", "fp32"), run(fscp, "--hip_precision", "fp32")
    assert wav == fm and [ln.split()[0] for ln in wav] == ["spk-utt%02d" % b for b in range(4)]


# ------------------------------------------------------------------------------------------------- 4. frame skipping
def test_archive_with_left_right_context_and_skip_3(tmp_path, monkeypatch):
    """(left, right, skip) = (1, 1, 3) on an `FM ` archive whose lengths are no multiples of 3: zero rows behind the CMVN, the right
    edge replicating them.  Three blocks of an 80-column archive are 240 values, so the model reads input_size 240 (no column count
    gives 80), and the reference's agreement formula, (1 + 1 + 1) // 3 x n_features, then wants n_features = 240."""
    counts = [61, 37, 50, 44, 58, 40, 47]
    assert all(n % 3 for n in counts)
    args, state = tiny240(left_ctx=1, right_ctx=1, skip_frame=3, n_features=240)
    mats = feature_mats(counts)
    scp = fm_archive(tmp_path, mats)
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, tmp_path, mats))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    packed = run(scp, "--hip_precision", "fp32")
    assert packed == run(scp, "--hip_precision", "fp32", "--hip_packed_reader", 0) == run(scp, "--hip_precision", "fp32", "--hip_pipelines", 1)
    assert run.stats[0]["spliced_passes"] == run.stats[0]["passes"] >= 1 and run.stats[1]["spliced_passes"] == 0
    assert len(packed) == len(counts) and all(len(ln.split()) > 1 for ln in packed)


def test_audio_with_right_context_and_skip_2_at_input_size_80(tmp_path, monkeypatch):
    """(0, 1, 2) on audio at input_size 80: 40 mel bins, two blocks, every second frame; odd frame counts.  n_features is 80 here,
    as the reference's formula ((0 + 1 + 1) // 2 x n_features = input_size) demands - not the mel count."""
    counts = [61, 37, 51, 45, 57, 39, 47]
    assert all(n % 2 for n in counts)
    args, state = tiny240(input_size=80, n_features=80, right_ctx=1, skip_frame=2)
    conf_file = tmp_path / "fbank.conf"
    conf_file.write_text("--num-mel-bins=40\n")
    wscp, fscp, mats = wave_twins(tmp_path, counts, num_mel=40)
    assert mats[0].shape == (61, 40)
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, tmp_path, mats, dim=40))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    fb = ["--hip_fbank_conf", str(conf_file), "--hip_precision", "fp32"]
    wav, fm = run(wscp, *fb), run(fscp, *fb)
    assert wav == fm and len(wav) == len(counts) and all(len(ln.split()) > 1 for ln in wav)
    assert wav == run(wscp, "--hip_pipelines", 1, *fb) == run(fscp, "--hip_packed_reader", 0, *fb)
    s = run.stats
    assert s[0]["wave_passes"] == s[0]["spliced_passes"] == s[0]["passes"] >= 1 and s[1]["spliced_passes"] == s[1]["passes"] >= 1, s


# ------------------------------------------------------------------------------------------------- 5. the engine at input_size 240
def spliced_batch(batch, lengths, triple=(0, 2, 1)):
    """Host-spliced features of a padded (B, T, 80) batch -> (B, T, 240), padding 0."""
    out = np.zeros((batch.shape[0], batch.shape[1], (triple[0] + triple[1] + 1) * batch.shape[2]), np.float32)
    for b, n in enumerate(lengths):
        out[b, :n] = splice_host(batch[b, :n], triple)
    return out


_oracle = {}


def tiny240_oracle():
    if not _oracle:
        args, state = tiny240()
        feats, sizes = synth.make_feats(3, 61, 80, lengths=[61, 50, 37], seed=11)
        feats = spliced_batch(feats, [61, 50, 37])
        _oracle["case"] = (args, state, feats, sizes, orc.decode_nast(state, feats, sizes, args, stages=True))
    return _oracle["case"]


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_tiny_engine_at_input_size_240_against_the_oracle(prec, capsys):
    """The gates test_gpu_pipeline applies to the tiny case at 80: hypotheses token for token, log-posteriors within LOGIT_TOL.
    bf16x3 as its parity gate there: an arg-max may differ only on a frame whose reference margin is below 1e-4, and the
    hypotheses are compared when none did."""
    _, state, feats, sizes, ref = tiny240_oracle()
    args, _ = tiny240()  # (build() writes the engine switches into it)
    model = build(args, state, prec, capture=True)
    out = decode(model, args, feats, sizes)
    eng = model._engine
    err = maxerr(eng.fetch("ctc_out"), ref["ctc_out"].numpy())
    flips = (eng.fetch("best_paths") != ref["best_paths"]) & ref["src_mask"].squeeze(1).numpy().astype(bool)  # (valid frames)
    with capsys.disabled():
        print(f"\n[input_size 240, {prec}] ctc_out max error {err:.3g}, arg-max flips {int(flips.sum())} of {flips.size}")
    assert err < LOGIT_TOL
    if prec == "fp32":
        assert not flips.any()
    assert (ref["ctc_margin"][flips] < 1e-4).all()
    if not flips.any():
        np.testing.assert_array_equal(eng.fetch("ylen"), ref["ylen"])
        assert [s[0]["hyp"] for s in out] == [list(h) for h in ref["hyps"]]
        np.testing.assert_allclose([s[0]["score"] for s in out], ref["scores"], atol=1e-3)


def test_config2_width_engine_at_input_size_240_bf16_against_fp32(capsys):
    """d_model 256 (the 256-channel conv kernels; conv1 on its VALU form: F1 = 120 > 63), N_enc 2, B = 2, T = 100: the bf16 engine
    against the fp32 engine - finite outputs, no arg-max flip on a frame whose fp32 top-2 margin is >= 0.05 (the gate of
    test_bf16_agreement_report)."""
    args = synth.make_args("config1", input_size=240, n_features=80, right_ctx=2)
    state = synth.make_state(args, seed=1, blank_bias=0.0)
    raw, sizes = synth.make_feats(2, 100, 80, lengths=[100, 83], seed=21)
    feats = spliced_batch(raw, [100, 83])
    got = {}
    for prec in ("fp32", "bf16"):
        model = build(args, state, prec, capture=True)
        out = decode(model, args, feats, sizes)
        eng = model._engine
        got[prec] = (eng.fetch("ctc_out"), eng.fetch("best_paths"), out)
    ctc32, best32, _ = got["fp32"]
    ctc16, best16, out16 = got["bf16"]
    assert np.isfinite(ctc32).all() and np.isfinite(ctc16).all()
    assert all(np.isfinite(s[0]["score"]) and len(s[0]["hyp"]) > 1 for s in out16)
    top2 = np.sort(ctc32, -1)[..., -2:]
    margin = top2[..., 1] - top2[..., 0]
    valid = np.zeros(best32.shape, bool)
    for b, n in enumerate([100, 83]):
        valid[b, : ((n - 1) // 2 + 1 - 1) // 2 + 1] = True
    flips = (best32 != best16) & valid
    with capsys.disabled():
        print(f"\n[input_size 240, d_model 256, bf16 vs fp32] ctc_out max diff {maxerr(ctc16[valid], ctc32[valid]):.3g}, flips "
              f"{int(flips.sum())} of {int(valid.sum())}, largest flip margin {float(margin[flips].max()) if flips.any() else 0.0:.3g}")
    assert not (flips & (margin >= 0.05)).any()
