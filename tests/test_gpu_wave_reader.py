"""Audio input on the device: cn_op_fbank_packed (int16 samples staged as the WAV files hold them -> padded fbank batch) against
cn_fbank bit for bit and the float64 oracle, its float64 CMVN against cn_op_cmvn bit for bit, and decode_asr end to end from a
`wav.scp` against the `FM ` archive of the same device features."""
import struct

import numpy as np
import pytest
import torch

from conftest import ast_tiny_case, tiny_case
from oracle import fbank_oracle as fo
from test_fbank import synth_wave
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.data import kaldi_io
from cassnat_asr_public_amd.data.fbank import Fbank

pytestmark = pytest.mark.gpu

SAMPLES = [400, 559, 560, 6935, 16160, 6800]  # 1, 1, 2, 41, 99, 41 frames at the default options; 559 and 6935 are odd
OPTS = [dict(), dict(window="povey", num_mel=40, low_freq=60.0, high_freq=-400.0),
        dict(preemph=0.0, remove_dc=0, frame_length_ms=20.0, window="hanning")]
PAD = -1.5


def int16_wave(n, seed):
    w = synth_wave(1.2, seed)[:n].astype(np.float64)
    if seed == 3:  # runs at both ends of the int16 range
        w[100:140], w[300:340] = -40000.0, 40000.0
    x = np.clip(np.rint(w), -32768, 32767).astype("<i2")
    assert len(x) == n
    return x


_waves = {}


def waves():
    if not _waves:
        _waves["w"] = [int16_wave(n, i) for i, n in enumerate(SAMPLES)]
        assert _waves["w"][3].min() == -32768 and _waves["w"][3].max() == 32767
    return _waves["w"]


def stage(views, lead=0):
    """The views at 16-byte-aligned offsets behind ``lead`` bytes, the gaps filled with noise -> (staged cuda bytes, total, off, ns)."""
    offs, total = hip.gather_offsets([v.nbytes for v in views], 16)
    offs = offs.astype(np.int64) + lead
    total += lead
    host = np.random.default_rng(5).integers(0, 256, size=total).astype(np.uint8)
    for o, v in zip(offs, views):
        host[o:o + v.nbytes] = v.view(np.uint8)
    return (torch.from_numpy(host).cuda(), total, torch.tensor(offs, dtype=torch.int32, device="cuda"),
            torch.tensor([len(v) for v in views], dtype=torch.int32, device="cuda"))


def run_packed(fb, views, T, mean=None, std=None, lead=0):
    staged, total, off, ns = stage(views, lead)
    out = torch.full((len(views), T, fb.o.num_mel), 7.0, device="cuda")
    hip.fbank_packed(fb.o, staged, total, off, ns, out, PAD, mean, std)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("with_cmvn", [False, True])
@pytest.mark.parametrize("opts", OPTS, ids=["default", "povey40", "hanning20ms"])
def test_fbank_packed_is_cn_fbank_on_int16_samples(opts, with_cmvn):
    ws = waves()
    fb = Fbank(**opts)
    frames = [fb.num_frames(len(w)) for w in ws]
    if not opts:
        assert frames == [1, 1, 2, 41, 99, 41]
    T = max(frames) + 3
    plain = run_packed(fb, ws, T)
    got = plain.cpu().numpy()
    if not with_cmvn:
        ref, _ = fb([w.astype(np.float32) for w in ws])  # cn_fbank on float32 copies of the same samples
        ref = ref.cpu().numpy()
        oo = {k: (bool(v) if k == "remove_dc" else v) for k, v in opts.items()}
        for b, (w, n) in enumerate(zip(ws, frames)):
            np.testing.assert_array_equal(got[b, :n], ref[b, :n])
            orc = fo.fbank(w.astype(np.float64), **oo)
            assert orc.shape[0] == n
            np.testing.assert_allclose(got[b, :n], orc, atol=2e-3, rtol=0)
            assert (got[b, n:] == np.float32(PAD)).all()
        # the utterances in another order, at other offsets: the same rows
        order = [4, 0, 5, 2, 1, 3]
        again = run_packed(fb, [ws[i] for i in order], T, lead=48).cpu().numpy()
        for j, i in enumerate(order):
            np.testing.assert_array_equal(again[j], got[i])
        return
    rng = np.random.default_rng(11)
    F = fb.o.num_mel
    mean, std = torch.from_numpy(rng.standard_normal(F) * 3 + 12).cuda(), torch.from_numpy(rng.random(F) + 0.5).cuda()
    normed = run_packed(fb, ws, T, mean, std).cpu().numpy()
    want = hip.cmvn_(plain.clone(), torch.tensor(frames, dtype=torch.int32, device="cuda"), mean, std)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(normed, want.cpu().numpy())
    for b, n in enumerate(frames):
        assert (normed[b, n:] == np.float32(PAD)).all() and not (normed[b, :n] == got[b, :n]).all()


def test_fbank_packed_refusals_leave_the_output_alone():
    L = hip.lib()
    fb = Fbank()
    staged, total, off, ns = stage(waves()[:2])
    out = torch.full((2, 4, 80), 7.0, device="cuda")
    st = hip.current_stream()
    p = hip._ptr

    def refused(*args):
        rc = L.cn_op_fbank_packed(*args)
        return rc != 0 and len(L.cn_last_error()) > 0

    assert refused(None, p(staged), total, p(off), p(ns), p(out), 2, 4, 0.0, None, None, st)
    assert refused(fb.o, None, total, p(off), p(ns), p(out), 2, 4, 0.0, None, None, st)
    assert refused(fb.o, p(staged), total, None, p(ns), p(out), 2, 4, 0.0, None, None, st)
    assert refused(fb.o, p(staged), total, p(off), None, p(out), 2, 4, 0.0, None, None, st)
    assert refused(fb.o, p(staged), total, p(off), p(ns), None, 2, 4, 0.0, None, None, st)
    assert refused(fb.o, p(staged), total, p(off), p(ns), p(out), 0, 4, 0.0, None, None, st)
    assert refused(fb.o, p(staged), total, p(off), p(ns), p(out), 2, 0, 0.0, None, None, st)
    assert refused(fb.o, p(staged), total, p(off), p(ns), p(out), 2, 4, 0.0, p(torch.zeros(80, dtype=torch.float64, device="cuda")), None, st)
    long_frame = Fbank(frame_length_ms=40.0)  # 640 samples > 512
    with pytest.raises(hip.HipError, match="512"):
        hip.fbank_packed(long_frame.o, staged, total, off, ns, out, 0.0)
    no_mel = Fbank()
    no_mel.o.num_mel = 0
    assert refused(no_mel.o, p(staged), total, p(off), p(ns), p(out), 2, 4, 0.0, None, None, st)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------- end to end
def write_wav(path, x):
    data = np.ascontiguousarray(x, dtype="<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, 16000, 32000, 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"LIST" + struct.pack("<I", 4) + b"INFO" + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


def twin_sets(tmp_path, frame_counts):
    """WAV files of the given frame counts (plus a few samples that complete no frame) and the `FM ` archive of the features the
    device computes from them (Fbank.packed, no CMVN) -> (wav.scp, feats.scp, the matrices)."""
    views, lines = [], []
    for b, n in enumerate(frame_counts):
        x = int16_wave(400 + 160 * (n - 1) + (37 * b) % 160, 20 + b)
        views.append(x)
        lines.append("spk-utt%02d %s\n" % (b, write_wav(tmp_path / ("utt%02d.wav" % b), x)))
    wscp = tmp_path / "wav.scp"
    wscp.write_text("".join(lines))
    feats, ratios = Fbank().packed(views)
    torch.cuda.synchronize()
    feats = feats.cpu().numpy()
    assert [round(float(r) * feats.shape[1]) for r in ratios] == list(frame_counts)
    mats = [("spk-utt%02d" % b, feats[b, :n].copy()) for b, n in enumerate(frame_counts)]
    fscp = str(tmp_path / "feats.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "feats.ark"), fscp, mats)
    return str(wscp), fscp, [m for _, m in mats]


def cmvn_stats(tmp_path, mats, dim):
    allf = np.vstack(mats).astype(np.float64)
    stats = np.zeros((2, dim + 1))
    stats[0, :-1], stats[0, -1], stats[1, :-1] = allf.sum(0), len(allf), (allf ** 2).sum(0)
    kaldi_io.write_ark_scp(str(tmp_path / "cmvn.ark"), str(tmp_path / "cmvn.scp"), [("global", stats)])
    return kaldi_io.read_scp(str(tmp_path / "cmvn.scp"))[0][1]


NAT_KEYS = ("input_size", "d_model", "n_head", "d_encff", "d_decff", "d_ff", "N_enc", "N_extra", "N_self_dec", "N_mix_dec", "model_type",
            "n_features", "left_ctx", "right_ctx", "skip_frame", "padding_idx", "beam_width", "length_penalty", "use_trigger")


def write_model(tmp_path, args, state, conf):
    import yaml

    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("".join(f"w{i}\n" for i in range(args.vocab_size - 4)))
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {"module." + k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    conf = dict(conf, vocab_file=str(vocab_file), use_gpu=True)
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))
    return ckpt, str(cfg)


@pytest.mark.parametrize("with_cmvn,pipelines,precision", [(False, 2, "fp32"), (True, 2, None), (True, 1, "fp32"), (False, 1, None)])
def test_cassnat_decode_from_a_wav_scp(tmp_path, monkeypatch, with_cmvn, pipelines, precision):
    """decode_asr on the tiny model from seven WAV files (batch size 3: the pipelined path with --hip_pipelines 2, the plain loop
    with 1) equals decoding the `FM ` archive of the same device features, line for line, with and without a global CMVN."""
    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.tasks import CassNATTask

    args, state, _, _ = tiny_case()
    counts = [61, 37, 50, 44, 58, 39, 47]
    wscp, fscp, mats = twin_sets(tmp_path, counts)
    conf = {k: getattr(args, k) for k in NAT_KEYS}
    if with_cmvn:
        conf.update(use_cmvn=True, global_cmvn=cmvn_stats(tmp_path, mats, 80))
    ckpt, cfg = write_model(tmp_path, args, state, conf)
    seen = []
    orig = CassNATTask.decode

    def decode(self, a):
        rc = orig(self, a)
        seen.append(dict(getattr(self, "pipeline_stats", None) or {}))
        self.pipeline_stats = None
        return rc

    monkeypatch.setattr(CassNATTask, "decode", decode)
    out = {}
    for name, scp in (("wav", wscp), ("fm", fscp)):
        result = str(tmp_path / f"res_{name}.txt")
        argv = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                "--batch_size", "3", "--load_data_workers", "0", "--hip_pipelines", str(pipelines)]
        assert decode_asr.main(argv + (["--hip_precision", precision] if precision else [])) == 0
        out[name] = open(result).read().splitlines()
    assert [ln.split()[0] for ln in out["wav"]] == ["spk-utt%02d" % b for b in range(len(counts))]
    assert out["wav"] == out["fm"]
    if pipelines > 1:
        assert seen[0]["wave_passes"] >= 1 and seen[0]["wave_passes"] == seen[0]["passes"] and seen[1]["wave_passes"] == 0, seen
    else:
        assert not seen[0]


def test_cassnat_ctc_only_from_a_wav_scp(tmp_path):
    """decode_type ctc_only goes through the plain loop: a WaveBatch becomes features there (BaseTask.wave_features)."""
    from cassnat_asr_public_amd.bin import decode_asr

    args, state, _, _ = tiny_case()
    wscp, fscp, _ = twin_sets(tmp_path, [61, 50, 37, 44])
    conf = {k: getattr(args, k) for k in NAT_KEYS}
    conf.update(decode_type="ctc_only", sample_num=1, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0)
    ckpt, cfg = write_model(tmp_path, args, state, conf)
    out = {}
    for name, scp in (("wav", wscp), ("fm", fscp)):
        result = str(tmp_path / f"res_{name}.txt")
        assert decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                                "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0"]) == 0
        out[name] = open(result).read().splitlines()
    assert out["wav"] == out["fm"] and len(out["wav"]) == 4


def test_art_decode_from_a_wav_scp(tmp_path):
    """ArtTask, ctc_att beam 3: its workers turn the WaveBatch into features on their own streams; equals the `FM ` twin."""
    from cassnat_asr_public_amd.bin import decode_asr

    args, state, _ = ast_tiny_case(ctc_weight=0.3)
    wscp, fscp, _ = twin_sets(tmp_path, [61, 57, 51, 40])
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight",
                                          "max_decode_ratio", "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(n_features=80, model_type="transformer", beam_width=3, decode_type="ctc_att")
    ckpt, cfg = write_model(tmp_path, args, state, conf)
    out = {}
    for name, scp in (("wav", wscp), ("fm", fscp)):
        result = str(tmp_path / f"res_{name}.txt")
        assert decode_asr.main(["--task", "art", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--result_file", result,
                                "--batch_size", "2", "--hip_precision", "fp32", "--load_data_workers", "0"]) == 0
        out[name] = open(result).read().splitlines()
    assert out["wav"] == out["fm"] and [ln.split()[0] for ln in out["wav"]] == ["spk-utt%02d" % b for b in range(4)]


def test_model_and_front_end_must_agree_on_the_feature_count(tmp_path):
    from cassnat_asr_public_amd.bin import decode_asr

    args, state, _, _ = tiny_case()
    wscp, _, _ = twin_sets(tmp_path, [40, 41])
    ckpt, cfg = write_model(tmp_path, args, state, {k: getattr(args, k) for k in NAT_KEYS})
    conf = tmp_path / "fbank.conf"
    conf.write_text("--num-mel-bins=40\n")
    with pytest.raises(ValueError, match="40.*80"):
        decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", wscp, "--resume_model", ckpt,
                         "--result_file", str(tmp_path / "r.txt"), "--hip_fbank_conf", str(conf)])
