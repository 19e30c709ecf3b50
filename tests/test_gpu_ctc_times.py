"""CTC token time stamps end to end.  Engine level: ``Engine.ctc_token_times`` against the numpy model (tests/ctc_times_model.py) run on
the engine's OWN log-posteriors - ``ctc_out`` of a capture run of ``ctc_beam`` on the same features - exact in every field, for fp32,
bf16x3, bf16 and fp16 engines, a CASS-NAT handle and an autoregressive handle with a CTC head.  CLI level: ``decode_asr --hip_ctm``
with ``--task cassnat`` and ``--task art`` on a tiny archive: the result file is byte-identical to the run without the flag, the
CTM words are the detokenised result lines, times are ordered and inside the utterance, confidences are probabilities."""
import numpy as np
import pytest
import torch

import ctc_times_cases as cases
import ctc_times_model as tm
from conftest import ast_tiny_case, ctcbeam_case, tiny_case
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.utils import ctm

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "bf16x3", "bf16", "fp16"]


def nat_model(which, prec):
    from test_gpu_ctcbeam import build

    args, state, feats, sizes = tiny_case() if which == "tiny" else ctcbeam_case("ctcbeam_tiny")
    return build(args, state, prec, capture=True), args, feats, sizes


def ast_model(prec):
    from cassnat_asr_public_amd.models.transformer import make_model

    args, state, feats = ast_tiny_case(ctc_weight=0.3)
    args.hip_precision, args.hip_capture = prec, True
    model = make_model(args.input_size, args).cuda()
    with torch.no_grad():
        for k, q in model.named_parameters():
            q.copy_(torch.from_numpy(state[k]))
    return model, args, feats, np.ones(feats.shape[0], np.float32)


def check_engine(model, args, feats, sizes):
    src, ratio = torch.from_numpy(feats).cuda(), torch.from_numpy(np.asarray(sizes, np.float32)).cuda()
    B, T, _ = src.shape
    eng = model.engine(B, T)
    opts = hip.Engine.make_opts(args, capture=True)
    hyp, hlen, *_ = eng.ctc_beam(src, ratio, opts, 5, 8, 0.2)
    ctc = np.asarray(eng.fetch("ctc_out"), np.float32)                 # the log-posteriors this engine computes for these features
    frames = eng.fetch("keymask").astype(bool).sum(1)
    assert ctc.shape[0] == B and frames.max() == ctc.shape[1]
    hyp, hlen = hyp.cpu().numpy(), hlen.cpu().numpy()
    best = [hyp[b, 0, :hlen[b, 0]].tolist() for b in range(B)]
    assert any(len(y) >= 2 for y in best)
    # the best hypotheses; then rows the search did not produce: reversed, too long for the frames, holding the blank
    tries = [best, [y[::-1] for y in best], [best[0], list(range(1, 4)) * ctc.shape[1], best[-1][:1] + [args.padding_idx]][:B]]
    for rows in tries:
        ld = max(1, max(len(y) for y in rows)) + 2
        labels = np.full((B, ld), cases.SENT_I, np.int32)
        for b, y in enumerate(rows):
            labels[b, :len(y)] = y
        llen = np.array([len(y) for y in rows], np.int32)
        got = eng.ctc_token_times(src, ratio, opts, torch.from_numpy(labels), torch.from_numpy(llen))
        start, end, conf, score, status = (t.cpu().numpy() for t in got)
        assert np.array_equal(np.asarray(eng.fetch("ctc_out"), np.float32), ctc)   # the second pass computed the same rows
        for b, y in enumerate(rows):
            w = tm.align(ctc[b], int(frames[b]), y, args.padding_idx)
            L = len(y)
            assert int(status[b]) == w["status"], b
            assert start[b, :L].tolist() == w["start"] and end[b, :L].tolist() == w["end"], (b, w)
            assert np.array_equal(cases.bits(conf[b, :L]), cases.bits(w["conf"])), b
            assert cases.bits(np.float64(score[b])) == cases.bits(np.float64(w["score"])), (b, score[b], w["score"])
            assert (start[b, L:] == -1).all() and (end[b, L:] == -1).all() and (conf[b, L:] == 0).all()
    assert [int(s) for s in status] == [0, 1, 2][:B]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["tiny", "ctcbeam_tiny"])
def test_engine_on_a_nat_handle_is_the_model_on_its_own_log_posteriors(which, prec):
    check_engine(*nat_model(which, prec))


@pytest.mark.parametrize("prec", PRECS)
def test_engine_on_an_ast_handle_is_the_model_on_its_own_log_posteriors(prec):
    check_engine(*ast_model(prec))


def test_refusals_of_the_model_entry():
    from cassnat_asr_public_amd.models.lm import make_model as make_lm
    from cassnat_asr_public_amd import synth

    model, args, feats, sizes = nat_model("tiny", "fp32")
    src, ratio = torch.from_numpy(feats).cuda(), torch.from_numpy(sizes).cuda()
    eng = model.engine(*src.shape[:2])
    opts = hip.Engine.make_opts(args)
    lab, llen = torch.ones(3, 4, dtype=torch.int32), torch.ones(3, dtype=torch.int32)
    with pytest.raises(hip.HipError, match="ld must"):
        eng.ctc_token_times(src, ratio, opts, torch.ones(3, 1501, dtype=torch.int32), llen)
    eng.ctc_token_times(src, None, opts, lab, llen)  # (size ratios are not read)
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=args.vocab_size)
    lm_args.hip_precision = "fp32"
    lm = make_lm(lm_args).cuda()
    with pytest.raises(hip.HipError, match="CTC head"):
        lm.step_engine(3).ctc_token_times(src, ratio, opts, lab, llen)


# ---- decode_asr --hip_ctm -------------------------------------------------------------------------------------------------------------
def read_ctm(path):
    out = {}
    for line in open(path, encoding="utf-8").read().splitlines():
        utt, chan, start, dur, word, conf = line.split(" ")
        assert chan == "1" and len(start.split(".")[1]) == 2 and len(dur.split(".")[1]) == 2 and len(conf.split(".")[1]) == 3, line
        out.setdefault(utt, []).append((float(start), float(dur), word, float(conf)))
    return out


def check_ctm(path, lines, lengths, detok, sec=0.04):
    got = read_ctm(path)
    assert any(len(ln.split()) > 2 for ln in lines)
    for ln, frames in zip(lines, lengths):
        utt, pieces = ln.split()[0], ln.split()[1:]
        words = got.get(utt, [])
        assert [w for _, _, w, _ in words] == detok(pieces), utt          # (an empty hypothesis has no lines)
        t, n = 0.0, hip.subsampled(frames)
        for start, dur, _, conf in words:
            # times in hundredths of a second: non-decreasing, not overlapping (up to the rounding of start and duration)
            assert start >= t - 0.0101 and dur > 0 and 0.0 <= conf <= 1.0, (utt, words)
            t = start + dur
        assert t <= n * sec + 0.0101, (utt, t, n)
    assert set(got) <= {ln.split()[0] for ln in lines}


def run_cli(tmp, cli, tag, flags=()):
    from cassnat_asr_public_amd.bin import decode_asr

    result = str(tmp / ("result_%s.txt" % tag))
    assert decode_asr.main(cli + ["--result_file", result] + list(flags)) == 0
    return open(result, "rb").read()


@pytest.mark.parametrize("decode_type", ["att_only", "ctc_att"])
def test_decode_asr_cassnat_writes_a_ctm_file_and_the_same_result_file(tmp_path, decode_type):
    """A vocabulary with separator pieces: words are merged pieces.  att_only would take the pipelined path; the flag keeps the plain loop."""
    from test_gpu_ctc_ngram import PIECES40
    from test_gpu_multirank import _write_case

    args, state, feats, sizes = tiny_case(decode_type=decode_type, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0)
    assert args.vocab_size == 40
    vocab_file = tmp_path / "pieces.txt"
    vocab_file.write_text("".join(p + "\n" for p in PIECES40[4:]), encoding="utf-8")
    lengths = [61, 50, 37, 61, 44]
    feats5 = np.concatenate([feats, feats[:2]])
    feats5[3, 50:], feats5[4, 44:] = 0, 0
    conf = dict(decode_type=decode_type, sample_num=1, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0, vocab_file=str(vocab_file))
    scp, ckpt, cfg = _write_case(tmp_path, args, state, feats5, lengths, extra_conf=conf)
    cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "2", "--hip_precision", "fp32",
           "--load_data_workers", "0"]
    plain = run_cli(tmp_path, cli, "plain")
    out = str(tmp_path / "out.ctm")
    assert run_cli(tmp_path, cli, "ctm", ["--hip_ctm", out]) == plain
    lines = plain.decode("utf-8").splitlines()
    check_ctm(out, lines, lengths, lambda pieces: "".join(pieces).replace(ctm.SEP, " ").split())
    # per token on request: one line per piece, the pieces as they are
    tok = str(tmp_path / "tok.ctm")
    assert run_cli(tmp_path, cli, "tok", ["--hip_ctm", tok, "--hip_ctm_unit", "token"]) == plain
    check_ctm(tok, lines, lengths, lambda pieces: pieces)


@pytest.mark.parametrize("decode_type", ["ctc_att", "ctc_only"])
def test_decode_asr_art_writes_a_ctm_file_and_the_same_result_file(tmp_path, decode_type):
    """ArtTask: every worker aligns on its own engine and stream; the vocabulary has no separator pieces, so the file is per token."""
    from test_gpu_multirank import _write_case

    args, state, feats = ast_tiny_case(ctc_weight=0.3)
    lengths = [61, 57, 51]
    conf = dict(decode_type=decode_type, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0)
    scp, ckpt, cfg = _write_case(tmp_path, args, state, feats, lengths, extra_conf=conf, ast=True)
    cli = ["--task", "art", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "2", "--hip_precision", "fp32",
           "--load_data_workers", "0"]
    plain = run_cli(tmp_path, cli, "plain")
    out = str(tmp_path / "out.ctm")
    assert run_cli(tmp_path, cli, "ctm", ["--hip_ctm", out]) == plain
    check_ctm(out, plain.decode("utf-8").splitlines(), lengths, lambda pieces: pieces)
