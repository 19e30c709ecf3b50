"""Kaldi compressed archives on the device: cn_op_unpack_compressed against the host definition (PackedBatch.padded(), i.e.
kaldi_io.decompress: Kaldi's float32 arithmetic) bit for bit, and decode_asr end to end from a `CM` archive against the `FM `
archive of the decompressed values."""
import struct

import numpy as np
import pytest
import torch

from conftest import ast_tiny_case, tiny_case
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.data import kaldi_io
from cassnat_asr_public_amd.pipeline import PackedBatch

pytestmark = pytest.mark.gpu

LENS = [61, 1, 33, 64, 32, 47, 96, 8, 9]
NAMES = {1: "CM", 2: "CM2", 3: "CM3"}


def random_payload(rng, kind, rows, F):
    """A payload of random headers and random codes (not encoder output): every segment of format 1 and both ends of each occur."""
    head = struct.pack("<ffii", np.float32(rng.standard_normal() * 5), np.float32(rng.random() * 40 + 0.1), rows, F)
    if kind == 1:
        headers = np.sort(rng.integers(0, 65536, size=(F, 4)), axis=1).astype("<u2")
        codes = rng.integers(0, 256, size=(F, rows)).astype(np.uint8)
        codes.ravel()[: min(codes.size, 6)] = [0, 64, 65, 192, 193, 255][: min(codes.size, 6)]
        body = headers.tobytes() + codes.tobytes()
    elif kind == 2:
        body = rng.integers(0, 65536, size=(rows, F)).astype("<u2").tobytes()
    else:
        body = rng.integers(0, 256, size=(rows, F)).astype(np.uint8).tobytes()
    return NAMES[kind], rows, F, np.frombuffer(head + body, np.uint8)


@pytest.mark.parametrize("F", [100, 101, 200])
def test_unpack_compressed_walks_the_columns_in_chunks(F):
    """More than 96 columns: format 1 goes through the kernel's LDS tile in several chunks of columns (96 + 4, 96 + 5 on the
    scalar store path, 96 + 96 + 8) - the column headers are converted again per chunk and the tile is reused."""
    test_unpack_compressed_is_decompress_collate_and_cmvn_on_the_device(F, (1, 2, 3), True)
    test_unpack_compressed_is_decompress_collate_and_cmvn_on_the_device(F, (1,), False)


@pytest.mark.parametrize("with_cmvn", [True, False])
@pytest.mark.parametrize("kinds", [(1,), (2,), (3,), (1, 2, 3)], ids=["CM", "CM2", "CM3", "mixed"])
@pytest.mark.parametrize("F", [80, 7, 83, 1])
def test_unpack_compressed_is_decompress_collate_and_cmvn_on_the_device(F, kinds, with_cmvn):
    """cn_op_unpack_compressed: the staged payloads of a pass -> the padded batch, bit for bit the host's decompression (no fused
    multiply-add), float64 CMVN and padding.  T = 96 holds every utterance; T = 70 is no multiple of the kernel's 64-frame tile
    and shorter than the longest utterances: their lengths are clamped while the column stride stays the payload's own row
    count.  F = 80 with format 1 and row counts that are no multiple of 4 is the case where a misaligned column run or a
    contracted multiply-add would show.  The output is pre-filled with 7.0: unwritten padding shows."""
    rng = np.random.default_rng(1000 * F + 10 * sum(kinds) + with_cmvn)
    entries = [random_payload(rng, kinds[b % len(kinds)], n, F) for b, n in enumerate(LENS)]
    pb = PackedBatch.from_payloads(entries)
    assert pb.shape == (len(LENS), 96, F)
    mean, std = rng.standard_normal(F), rng.random(F) + 0.5
    want = pb.padded(-1.5, (mean, std) if with_cmvn else None).numpy()
    offs, total = hip.gather_offsets([v.nbytes for v in pb.views], 16)
    host = np.zeros(total, np.uint8)
    assert hip.host_gather(host.ctypes.data, pb.views, 2, align=16).tolist() == offs.tolist()
    staged = torch.from_numpy(host).cuda()
    off = torch.tensor(offs.astype(np.int64), dtype=torch.int32, device="cuda")
    ln = torch.tensor(pb.lens, dtype=torch.int32, device="cuda")
    kd = torch.tensor(pb.kinds, dtype=torch.int32, device="cuda")
    m, s = (torch.from_numpy(mean).cuda(), torch.from_numpy(std).cuda()) if with_cmvn else (None, None)
    for T in (96, 70):
        out = torch.full((len(LENS), T, F), 7.0, device="cuda")
        hip.unpack_compressed(staged, off, ln, kd, out, -1.5, m, s)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want[:, :T])


def test_unpack_compressed_refuses_bad_arguments():
    out = torch.zeros((2, 8, 4), device="cuda")
    i32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    staged = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.HipError, match="mean and std come together"):
        hip.unpack_compressed(staged, i32, i32, i32, out, 0.0, torch.zeros(4, dtype=torch.float64, device="cuda"), None)
    with pytest.raises(hip.HipError, match="16-byte"):
        hip.unpack_compressed(staged[1:], i32, i32, i32, out, 0.0)


def _cmvn_stats(tmp_path, mats, dim):
    allf = np.vstack(mats).astype(np.float64)
    stats = np.zeros((2, dim + 1))
    stats[0, :-1], stats[0, -1], stats[1, :-1] = allf.sum(0), len(allf), (allf ** 2).sum(0)
    kaldi_io.write_ark_scp(str(tmp_path / "cmvn.ark"), str(tmp_path / "cmvn.scp"), [("global", stats)])
    return kaldi_io.read_scp(str(tmp_path / "cmvn.scp"))[0][1]


def _twin_archives(tmp_path, raw):
    """The matrices as a `CM` archive, and the `FM ` archive of what that one decompresses to."""
    cscp, fscp = str(tmp_path / "c.scp"), str(tmp_path / "f.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "c.ark"), cscp, [(f"spk-utt{b}", m) for b, m in enumerate(raw)], compress=1)
    values = [(u, kaldi_io.load_mat(s)) for u, s in kaldi_io.read_scp(cscp)]
    kaldi_io.write_ark_scp(str(tmp_path / "f.ark"), fscp, values)
    assert {kaldi_io.mat_kind(s) for _, s in kaldi_io.read_scp(cscp)} == {"CM"}
    return cscp, fscp, [m for _, m in values]


def test_cassnat_decode_from_a_compressed_archive(tmp_path):
    """CassNATTask.decode on the tiny model (archive, config and lengths of test_decode_asr_cli_with_global_cmvn_on_the_device):
    from a `CM` archive with the defaults - the packed reader, payloads decompressed and normalised on the device - the result
    file equals the one from the `FM ` archive of the decompressed values; so do `--hip_packed_reader 0` (DataLoader, host
    decompression, device CMVN) and `--hip_pipelines 1` (the plain loop)."""
    import yaml

    from cassnat_asr_public_amd.tasks import CassNATTask
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    args, state, feats, sizes = tiny_case()
    lengths = [61, 50, 37, 61, 12]
    rng = np.random.default_rng(1)
    raw = [(rng.standard_normal((n, feats.shape[2])) * 2.5 + 0.7).astype(np.float32) for n in lengths]
    cscp, fscp, values = _twin_archives(tmp_path, raw)
    cmvn_spec = _cmvn_stats(tmp_path, values, feats.shape[2])
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("".join(f"w{i}\n" for i in range(args.vocab_size - 4)))
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {"module." + k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_encff", "d_decff", "d_ff", "N_enc", "N_extra",
                                          "N_self_dec", "N_mix_dec", "model_type", "n_features", "left_ctx", "right_ctx",
                                          "skip_frame", "padding_idx", "beam_width", "length_penalty", "use_trigger")}
    conf.update(vocab_file=str(vocab_file), use_gpu=True, use_cmvn=True, global_cmvn=cmvn_spec)
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))

    def task_on(scp):
        a = DecodeParser().get_args(["--task", "cassnat", "--test_config", str(cfg), "--data_path", scp, "--resume_model", ckpt,
                                     "--result_file", str(tmp_path / "res.txt"), "--batch_size", "1", "--hip_precision", "fp32",
                                     "--load_data_workers", "0"])
        for k, v in conf.items():
            setattr(a, k, v)
        a.test_paths = [{"name": "test", "scp_path": scp}]
        a.rank = 0
        return CassNATTask("test", a), a

    def run(task, a, name, **over):
        for k, v in over.items():
            setattr(a, k, v)
        a.result_file = str(tmp_path / name)
        task.decode(a)
        return open(a.result_file).read().splitlines()

    task, a = task_on(fscp)
    want = run(task, a, "f.txt")
    assert task.pipeline_stats["passes"] >= 1 and task.pipeline_stats["compressed_passes"] == 0 and task._pipes.cmvn is not None
    task.close()
    assert len(want) == len(lengths) and all(len(ln.split()) > 1 for ln in want)
    task, a = task_on(cscp)
    assert task.test_loader.dataset.can_defer_cmvn()
    got = run(task, a, "c.txt")
    stats = dict(task.pipeline_stats)
    assert stats["passes"] >= 1 and stats["compressed_passes"] == stats["passes"], stats  # every pass was staged compressed
    assert task._pipes.cmvn is not None  # normalised on the device
    assert got == want
    assert run(task, a, "c_loader.txt", hip_packed_reader=0) == want
    assert task.pipeline_stats["compressed_passes"] == 0 and task.pipeline_stats["passes"] >= 1
    assert run(task, a, "c_plain.txt", hip_packed_reader=1, hip_pipelines=1) == want
    task.close()


def test_art_decode_from_a_compressed_archive(tmp_path):
    """ArtTask (autoregressive beam search; it reads through the dataset, host decompression) from a `CM` archive equals its
    `FM ` twin."""
    import yaml

    from cassnat_asr_public_amd.bin import decode_asr

    args, state, feats = ast_tiny_case(ctc_weight=0.3)
    raw = [feats[b, :n] for b, n in enumerate([61, 57, 51])]
    cscp, fscp, _ = _twin_archives(tmp_path, raw)
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("".join(f"w{i}\n" for i in range(args.vocab_size - 4)))
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {"module." + k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight",
                                          "max_decode_ratio", "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(vocab_file=str(vocab_file), use_gpu=True, n_features=80, model_type="transformer")
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))
    out = {}
    for name, scp in (("c", cscp), ("f", fscp)):
        result = str(tmp_path / f"res_{name}.txt")
        rc = decode_asr.main(["--task", "art", "--test_config", str(cfg), "--data_path", scp, "--resume_model", ckpt,
                              "--result_file", result, "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0"])
        assert rc == 0
        out[name] = open(result).read().splitlines()
    assert out["c"] == out["f"] and [ln.split()[0] for ln in out["c"]] == [f"spk-utt{b}" for b in range(3)]


def test_cassnat_decode_from_plain_path_entries(tmp_path):
    """An .scp of plain paths (one float32 matrix per file, no `:offset`) on the default pipelined path - the float32 packed reader,
    whose payloads then come from load_mat - gives the result file of the same matrices in one archive."""
    import yaml

    from cassnat_asr_public_amd.bin import decode_asr

    args, state, feats, sizes = tiny_case()
    lengths = [61, 50, 37, 44]
    mats = [(f"spk-utt{b}", feats[b % 3, :n]) for b, n in enumerate(lengths)]
    ark_scp, plain_scp = str(tmp_path / "feats.scp"), str(tmp_path / "plain.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "feats.ark"), ark_scp, mats)
    with open(plain_scp, "w") as f:
        for utt, m in mats:
            one = str(tmp_path / (utt + ".ark"))
            kaldi_io.write_ark_scp(one, str(tmp_path / "unused.scp"), [(utt, m)])
            f.write(f"{utt} {one}\n")
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("".join(f"w{i}\n" for i in range(args.vocab_size - 4)))
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {"module." + k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_encff", "d_decff", "d_ff", "N_enc", "N_extra",
                                          "N_self_dec", "N_mix_dec", "model_type", "n_features", "left_ctx", "right_ctx",
                                          "skip_frame", "padding_idx", "beam_width", "length_penalty", "use_trigger")}
    conf.update(vocab_file=str(vocab_file), use_gpu=True)
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))
    out = {}
    for name, scp in (("plain", plain_scp), ("ark", ark_scp)):
        result = str(tmp_path / f"res_{name}.txt")
        rc = decode_asr.main(["--task", "cassnat", "--test_config", str(cfg), "--data_path", scp, "--resume_model", ckpt,
                              "--result_file", result, "--batch_size", "1", "--hip_precision", "fp32", "--load_data_workers", "0"])
        assert rc == 0
        out[name] = open(result).read().splitlines()
    assert out["plain"] == out["ark"] and len(out["ark"]) == len(lengths)
