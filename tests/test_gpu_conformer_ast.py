"""GPU parity of the conformer AST model (src/models/conformer.py: conformer encoder, transformer decoder with Swish FFNs)
through the drop-in ``models.conformer`` API - an engine with ast = 1, conf_enc = 1 - and of the Swish forms of the fused
feed-forward kernels.  Goldens are the reference's own outputs (tests/golden/conf_ast_*.npz, conf_art_tiny_*.npz,
esa_at_conf_tiny.npz; tools/make_conformer_ast_goldens.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models.conformer import make_model

pytestmark = pytest.mark.gpu

SWISH = 1  # CN_ACT_SWISH


class Vocab:
    word2index = {"blank": 0, "sos": 1, "eos": 2, "unk": 3}
    index2word = {i: f"▁w{i}" for i in range(64)}


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def relerr(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------- the fixtures' seeded inputs
def tiny_case(**ov):
    args = synth.make_args_ast("tiny_conf_ast", beam_width=3, ctc_beam=5, max_decode_ratio=0.5, **ov)
    state = synth.make_state(synth.make_args_ast("tiny_conf_ast"), seed=3, gain=2.0)
    feats, _ = synth.make_feats(3, 61, 80, lengths=[61, 57, 51], seed=11)
    return args, state, feats


def c4_case():
    args = synth.make_args_ast("config4_conf", N_enc=3, max_decode_ratio=0.3, ctc_weight=0.3)
    state = synth.make_state(args, seed=5)
    feats, _ = synth.make_feats(4, 300, 80, lengths=[300, 287, 262, 231], seed=31)
    return args, state, feats


def art_case(bw):
    args = synth.make_args_ast("tiny_conf_ast", beam_width=bw, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0, length_penalty=0.1,
                               use_gpu=False, lm_weight=0)
    state = synth.make_state(synth.make_args_ast("tiny_conf_ast"), seed=3, gain=2.0)
    feats, sizes = synth.make_feats(3, 61, 80, lengths=[61, 57, 51], seed=11)
    return args, state, feats, sizes


def build(args, state, prec, host_beam=False):
    args.hip_precision = prec
    args.hip_host_beam = host_beam
    model = make_model(args.input_size, args).cuda()
    with torch.no_grad():
        for k, q in model.named_parameters():
            q.copy_(torch.from_numpy(state[k]))
    return model


def run(args, state, feats, prec, host_beam=False):
    model = build(args, state, prec, host_beam)
    src = torch.from_numpy(feats)
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    with torch.no_grad():
        return model.beam_decode(src.cuda(), mask.cuda(), Vocab, args)


def agreement(beams, g):
    exact, total, top1 = 0, 0, 0
    for b, utt in enumerate(beams):
        for j, s in enumerate(utt):
            ok = s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist()
            exact += ok
            total += 1
            top1 += ok and j == 0
    return exact, total, top1


# ---------------------------------------------------------------------------------------- Swish feed-forward kernels
def ffn_inputs(M, dff):
    g = torch.Generator().manual_seed(7 * M + dff)
    d = 256
    x = torch.randn(M, d, generator=g) * 2 + 0.3
    a, b = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    w1 = (torch.randn(dff, d, generator=g) / math.sqrt(d)).contiguous()
    b1 = 0.1 * torch.randn(dff, generator=g)
    w2 = (torch.randn(d, dff, generator=g) / math.sqrt(dff)).contiguous()
    b2 = 0.1 * torch.randn(d, generator=g)
    return x, a, b, w1, b1, w2, b2


def swish64(x, a, b, w1, b1, w2, b2, round16=False, act="swish"):
    """float64 numpy: x + W2 swish(W1 LN(x) + b1) + b2 (norm.py:15-18: unbiased std, eps on the std).  round16: the operands the
    bf16 kernel multiplies (LN output, weights, hidden activations) rounded to bf16 first."""
    r = (lambda t: t.to(torch.bfloat16).double().numpy()) if round16 else (lambda t: t.double().numpy())
    xd = x.double().numpy()
    mu = xd.mean(-1, keepdims=True)
    sd = xd.std(-1, ddof=1, keepdims=True)
    xn = a.double().numpy() * (xd - mu) / (sd + 1e-6) + b.double().numpy()
    xn = r(torch.from_numpy(xn))
    h = xn @ r(w1).T + b1.double().numpy()
    h = h / (1.0 + np.exp(-h)) if act == "swish" else np.maximum(h, 0.0)
    h = r(torch.from_numpy(h))
    return torch.from_numpy(xd + h @ r(w2).T + b2.double().numpy())


@pytest.mark.parametrize("dff", [1024, 2048])
@pytest.mark.parametrize("M", [1, 7, 64, 300])
@pytest.mark.parametrize("nslice", [1, 8])
def test_ffn_fused_swish_bf16(M, dff, nslice):
    """fused.hip with the Swish activation, whole rows and the decode step's d_ff split (+ ffn_reduce_kernel): against float64 on
    the operands rounded as the kernel rounds them."""
    x, a, b, w1, b1, w2, b2 = ffn_inputs(M, dff)
    ref = swish64(x, a, b, w1, b1, w2, b2, round16=True)
    xd, ad, bd, b1d, b2d = (t.contiguous().cuda() for t in (x, a, b, b1, b2))
    hip.check(hip.lib().cn_op_ffn_fused_act(p(xd), p(ad), p(bd), C.c_void_p(w1.data_ptr()), p(b1d), C.c_void_p(w2.data_ptr()),
                                            p(b2d), None, None, None, M, dff, C.c_float(1e-6), nslice, SWISH, hip.current_stream()))
    torch.cuda.synchronize()
    err = relerr(xd, ref)
    print(f"[ffn_fused swish] M {M} dff {dff} nslice {nslice}: relative error {err:.2e}")
    assert err < 2e-3  # accumulation order + the bf16 rounding of h (as the ReLU kernel's test)
    assert relerr(xd, swish64(x, a, b, w1, b1, w2, b2, round16=True, act="relu")) > 10 * err  # (and not the ReLU sublayer)


@pytest.mark.parametrize("dff", [1024, 2048])
@pytest.mark.parametrize("M", [1, 7, 64, 300])
def test_ffn_x3_swish_split_bf16(M, dff):
    """fused_x3.hip's plain split form with the Swish activation (three bf16 MFMAs per product on hi + lo operands): against float64
    on the unrounded operands."""
    x, a, b, w1, b1, w2, b2 = ffn_inputs(M, dff)
    ref = swish64(x, a, b, w1, b1, w2, b2)
    xd, ad, bd, b1d, b2d = (t.contiguous().cuda() for t in (x, a, b, b1, b2))
    hip.check(hip.lib().cn_op_ffn_x3_act(p(xd), p(ad), p(bd), C.c_void_p(w1.data_ptr()), p(b1d), C.c_void_p(w2.data_ptr()), p(b2d),
                                         None, None, None, M, dff, C.c_float(1e-6), 0, SWISH, hip.current_stream()))
    torch.cuda.synchronize()
    err = relerr(xd, ref)
    print(f"[ffn_x3 swish] M {M} dff {dff}: relative error {err:.2e}")
    assert err < 1e-5


def test_swish_is_refused_in_the_mixed_arithmetic():
    x, a, b, w1, b1, w2, b2 = ffn_inputs(7, 1024)
    xd, ad, bd, b1d, b2d = (t.contiguous().cuda() for t in (x, a, b, b1, b2))
    rc = hip.lib().cn_op_ffn_x3_act(p(xd), p(ad), p(bd), C.c_void_p(w1.data_ptr()), p(b1d), C.c_void_p(w2.data_ptr()), p(b2d),
                                    None, None, None, 7, 1024, C.c_float(1e-6), 1, SWISH, hip.current_stream())
    assert rc != 0 and b"mixed arithmetic" in hip.lib().cn_last_error()
    assert torch.equal(xd.cpu(), x)


# ------------------------------------------------------------------------------------------------ whole-model parity
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name,ov", [("conf_ast_tiny_att", dict(ctc_weight=0.0)), ("conf_ast_tiny_ctc", dict(ctc_weight=0.3))])
def test_conf_ast_tiny_all_beams(name, ov, prec):
    g = load_golden(name)
    args, state, feats = tiny_case(**ov)
    beams = run(args, state, feats, prec)
    for b, utt in enumerate(beams):
        assert len(utt) == args.beam_width
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)
            assert abs(s["score"] - g["beam_score"][b, j]) < max(5e-3, 1e-6 * abs(g["beam_score"][b, j]))


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_conf_ast_c4_beam10(prec, capsys):
    """d 256 / 6 decoder layers / d_decff 2048: the decode step's FFNs are the fused Swish kernels (bf16x3: the split form; the
    fp32 engine: the gemm epilogue), beam 10, ctc_weight 0.3, 22 steps."""
    g = load_golden("conf_ast_c4")
    args, state, feats = c4_case()
    beams = run(args, state, feats, prec)
    exact, total, top1 = agreement(beams, g)
    with capsys.disabled():
        print(f"\n[conformer AST {prec}] conf_ast_c4: {exact}/{total} beams identical, top-1 identical for {top1}/{len(beams)}")
    assert exact == total
    for b, utt in enumerate(beams):
        for j, s in enumerate(utt):
            assert abs(s["score"] - g["beam_score"][b, j]) < max(5e-3, 1e-6 * abs(g["beam_score"][b, j]))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_conf_ast_c4_half_precision_report(prec, capsys):
    """The 16-bit engines (bf16; fp16 from the second library, whose feature-range guard beam_decode checks): agreement reported,
    constrained loosely - a regression shows as beams falling apart."""
    g = load_golden("conf_ast_c4")
    args, state, feats = c4_case()
    beams = run(args, state, feats, prec)
    exact, total, top1 = agreement(beams, g)
    prefix = []
    for b, utt in enumerate(beams):
        ref = g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist()
        got = utt[0]["hyp"]
        k = 0
        while k < min(len(ref), len(got)) and ref[k] == got[k]:
            k += 1
        prefix.append(k)
        assert len(got) == len(ref) and np.isfinite(utt[0]["score"])
    with capsys.disabled():
        print(f"\n[conformer AST {prec}] beams identical {exact}/{total}, top-1 identical {top1}/{len(beams)}, common prefix of best {prefix}")
    # constrained at about half of what this build measures (bf16 31/40 beams, fp16 32/40; common prefixes of the best hypothesis
    # 16-23 tokens of 22, save one fp16 utterance whose third token is a near-tie below either engine's rounding)
    assert exact >= 16 and np.mean(prefix) >= 8


def test_conf_ast_device_beam_equals_host_beam_bf16():
    args, state, feats = c4_case()
    dev_b = run(args, state, feats, "bf16")
    host_b = run(args, state, feats, "bf16", host_beam=True)
    for u, v in zip(dev_b, host_b):
        assert [s["hyp"] for s in u] == [s["hyp"] for s in v]
        assert [s["score"] for s in u] == [s["score"] for s in v]


def test_conf_ast_host_beam_matches_golden():
    g = load_golden("conf_ast_tiny_ctc")
    args, state, feats = tiny_case(ctc_weight=0.3)
    beams = run(args, state, feats, "fp32", host_beam=True)
    for b, utt in enumerate(beams):
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("bw", [1, 3])
def test_conf_art_ctc_correct_and_ctc_only(bw, prec):
    from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode

    g = load_golden(f"conf_art_tiny_correct_bw{bw}")
    args, state, feats, sizes = art_case(bw)
    model = build(args, state, prec)
    src = torch.from_numpy(feats)
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    with torch.no_grad():
        beams = model.fast_decode_with_ctc(src.cuda(), mask.cuda(), Vocab, args)
    for b, utt in enumerate(beams):
        assert len(utt) == bw
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)
            assert abs(s["score"] - g["beam_score"][b, j]) < max(5e-3, 1e-6 * abs(g["beam_score"][b, j]))
    if bw == 1:
        with torch.no_grad():
            top = ctc_beam_decode(model, src.cuda(), mask.cuda(), torch.from_numpy(sizes).cuda(), Vocab, args, None)
        for b, seqs in enumerate(top):
            assert len(seqs) == int(g["ctc_n"][b])
            for j, s in enumerate(seqs):
                assert s["hyp"] == g["ctc_hyp"][b, j, : g["ctc_len"][b, j]].tolist(), (b, j)
            np.testing.assert_allclose([s["score_ctc"] for s in seqs], g["ctc_score"][b, : len(seqs)], rtol=0, atol=2e-3)


def test_esa_ranked_by_the_conformer_ast():
    """CassNAT ESA (sample_num 4) with rank_model 'at_baseline' on a conformer ranker: the hypotheses the reference picks (same
    tie rule as the transformer ranker's test)."""
    from cassnat_asr_public_amd.models.cassnat import make_model as make_cassnat

    g = load_golden("esa_at_conf_tiny")
    args = synth.make_args("tiny", sample_num=4, threshold=0.9, rank_model="at_baseline")
    state = synth.make_state(args, seed=0, gain=2.0)
    aa = synth.make_args_ast("tiny_conf_ast")
    ast_state = synth.make_state(aa, seed=3, gain=2.0)
    feats, sizes = synth.make_feats(3, 61, 80, lengths=[61, 50, 37], seed=11)
    args.esa_select = g["select"]
    args.hip_precision = "fp32"
    model = make_cassnat(args.input_size, args).cuda()
    with torch.no_grad():
        for k, q in model.named_parameters():
            q.copy_(torch.from_numpy(state[k]))
    ast = build(aa, ast_state, "fp32")
    src = torch.from_numpy(feats).cuda()
    with torch.no_grad():
        out, _ = model.beam_decode(src, (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(sizes).cuda(), Vocab, args, ast)
    for b, seqs in enumerate(out):
        h, ref = seqs[0]["hyp"], g["hyp"][b, : g["hyp_len"][b]].tolist()
        n = len(h) - 1 if len(h) == len(ref) and h[-1] == 0 and ref[-1] != 0 else len(h)  # the masked-row tie token
        assert len(h) == len(ref) and h[:n] == ref[:n]
    np.testing.assert_allclose([s[0]["score"] for s in out], g["score"], rtol=1e-5, atol=2e-3)


def test_decode_asr_cli_task_art_conformer(tmp_path):
    """decode_asr.py --task art with model_type conformer (ArtTask.set_model, src/tasks/art_task.py:32-35), fp32 engine: the result
    file holds the best beam of the reference's golden run."""
    import yaml

    from cassnat_asr_public_amd.bin import decode_asr
    from cassnat_asr_public_amd.data import kaldi_io

    g = load_golden("conf_ast_tiny_ctc")
    args, state, feats = tiny_case(ctc_weight=0.3)
    lengths = [61, 57, 51]
    mats = [(f"spk-utt{b}", feats[b, :n]) for b, n in enumerate(lengths)]
    scp = str(tmp_path / "feats.scp")
    kaldi_io.write_ark_scp(str(tmp_path / "feats.ark"), scp, mats)
    vocab_file = tmp_path / "vocab.txt"
    vocab_file.write_text("".join(f"w{i}\n" for i in range(args.vocab_size - 4)))
    ckpt = str(tmp_path / "model.mdl")
    torch.save({"model_state": {"module." + k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "d_decff", "N_enc", "N_dec", "ctc_weight",
                                          "max_decode_ratio", "T", "ctc_beam", "beam_width", "length_penalty", "decode_type",
                                          "use_conv_enc", "pos_type", "share_ff", "enc_max_relative_len", "enc_kernel_size")}
    conf.update(vocab_file=str(vocab_file), use_gpu=True, n_features=80, model_type="conformer")
    cfg = tmp_path / "decode.yaml"
    cfg.write_text(yaml.safe_dump(conf))
    result = str(tmp_path / "token_results.txt")
    rc = decode_asr.main(["--task", "art", "--test_config", str(cfg), "--data_path", scp, "--resume_model", ckpt,
                          "--result_file", result, "--batch_size", "3", "--hip_precision", "fp32", "--load_data_workers", "0"])
    assert rc == 0
    lines = open(result).read().splitlines()
    assert [ln.split()[0] for ln in lines] == [f"spk-utt{b}" for b in range(3)]
    for b, ln in enumerate(lines):
        best = g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist()
        eos_at = best.index(2) if 2 in best else len(best)
        assert ln.split()[1:] == [f"w{t - 4}" for t in best[:eos_at] if t not in (0, 1)], b
