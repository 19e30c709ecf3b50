"""Timing of the CTC token time stamps (cn_ctc_token_times, decode_asr --hip_ctm) on the bench workload: config 2, B utterances x 1000
frames (T' 250), synth.BENCH_BLANK_BIAS, bf16, the batch's greedy hypotheses as labels.  All legs run in one process and take turns,
`--runs` rounds after a warm-up; medians and ranges.  One JSON line, appended to --out (profiles/ctc_times_time.jsonl):

  1. the new launch alone (HIP events of the ProfScope tag ctc_token_times) beside the existing forced-alignment launch on the same
     labels (tag ctc_viterbi inside cn_decode_nast_forced: code this change does not touch), and their ratio;
  2. a whole Engine.ctc_token_times call per batch beside the encode pass it contains (Engine.encode_align: encoder, CTC head and the
     greedy alignment, the nearest existing entry);
  3. decode_asr's plain loop (--hip_pipelines 1, in process, an archive of --batches batches) with and without --hip_ctm, in utt/s.

    python tools/time_ctc_times.py [--batch 32] [--frames 1000] [--precision bf16] [--runs 5] [--batches 8]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cassnat_asr_public_amd import hip, synth  # noqa: E402
from cassnat_asr_public_amd.data import kaldi_io  # noqa: E402
from cassnat_asr_public_amd.models import make_cassnat_model  # noqa: E402
from cassnat_asr_public_amd.utils import ctm  # noqa: E402
from ragged_cli_bench import make_task  # noqa: E402
from time_ctc_lm import load  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "range": [round(min(xs), digits), round(max(xs), digits)]}


def engine_legs(a, args, state, rec):
    model = load(make_cassnat_model(args.input_size, args).cuda(), state)
    feats, sizes = synth.make_feats(a.batch, a.frames, args.input_size, seed=1234)
    src, ratio = torch.from_numpy(feats).cuda(), torch.from_numpy(sizes).cuda()
    V = args.vocab_size
    pieces = ["blank", "sos", "eos", "unk"] + ["w%d" % i for i in range(V - 4)]
    vocab = type("vocab", (), dict(index2word=dict(enumerate(pieces)), word2index={p: i for i, p in enumerate(pieces)}, n_words=V))
    with torch.no_grad():
        out, _ = model.beam_decode(src, None, ratio, vocab, args, None)
    ids = [ctm.label_ids(s[0]["hyp"], vocab, args.padding_idx) for s in out]
    B, ld = len(ids), max(1, max(len(y) for y in ids))
    labels = np.zeros((B, ld), np.int32)
    for b, y in enumerate(ids):
        labels[b, :len(y)] = y
    lab = torch.from_numpy(labels).cuda()
    llen = torch.tensor([len(y) for y in ids], dtype=torch.int32, device="cuda")
    eng = model.engine(B, a.frames)
    opts = hip.Engine.make_opts(args)
    Tp = hip.subsampled(a.frames)
    hyp = torch.empty(B, Tp + 2, dtype=torch.int32, device="cuda")
    hlen, score = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
    got = {}

    def times():
        got["t"] = eng.ctc_token_times(src, ratio, opts, lab, llen)

    legs = {"token_times_call": times, "forced_call": lambda: eng.decode_forced(src, ratio, opts, lab, llen, ld, hyp, hlen, score),
            "encode_align_call": lambda: eng.encode_align(src, ratio, opts)}
    for fn in legs.values():
        fn()
    calls = {k: [] for k in legs}
    launch = {"ctc_token_times": [], "ctc_viterbi": []}
    for _ in range(a.runs):
        eng.profile_begin(list(launch))
        for k, fn in legs.items():
            calls[k].append(wall(fn) * 1e3)
        prof = eng.profile_end()
        for tag in launch:
            launch[tag].append(prof[tag]["ms"] / prof[tag]["count"])
    status = got["t"][4].cpu().numpy()
    rec.update(labels_per_utt_mean=round(float(np.mean([len(y) for y in ids])), 1), label_row_width=ld, subsampled_frames=Tp,
               utterances_aligned=int((status == 0).sum()),
               token_times_launch_ms=stats(launch["ctc_token_times"]), viterbi_launch_ms=stats(launch["ctc_viterbi"]),
               token_times_over_viterbi=round(statistics.median(launch["ctc_token_times"]) / statistics.median(launch["ctc_viterbi"]), 3),
               token_times_call_ms=stats(calls["token_times_call"], 3), encode_align_call_ms=stats(calls["encode_align_call"], 3),
               forced_call_ms=stats(calls["forced_call"], 3),
               token_times_call_over_encode_align=round(statistics.median(calls["token_times_call"]) / statistics.median(calls["encode_align_call"]), 3))
    eng.close()
    model._engine = None


def cli_legs(a, margs, state, rec):
    utts = a.batch * a.batches
    with tempfile.TemporaryDirectory() as tmp:
        feats, _ = synth.make_feats(utts, a.frames, margs.input_size, seed=77)
        scp = os.path.join(tmp, "feats.scp")
        kaldi_io.write_ark_scp(os.path.join(tmp, "feats.ark"), scp, (("spk-utt%05d" % b, feats[b]) for b in range(utts)))
        vocab_file = os.path.join(tmp, "vocab.txt")
        with open(vocab_file, "w") as f:
            f.write("".join("w%d\n" % i for i in range(margs.vocab_size - 4)))
        ckpt = os.path.join(tmp, "model.mdl")
        torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, ckpt)
        keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
        conf = {k: getattr(margs, k) for k in keys}
        conf.update(vocab_file=vocab_file, use_gpu=True, test_paths=[{"name": "test", "scp_path": scp}])
        cfg = os.path.join(tmp, "decode.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump({k: v for k, v in conf.items() if k != "test_paths"}, f)
        base = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", str(a.batch),
                "--hip_precision", a.precision, "--hip_max_frames", str(a.frames), "--print_freq", "100000", "--hip_pipelines", "1",
                "--load_data_workers", "0"]
        tasks = {}
        for name, extra in (("plain", []), ("ctm", ["--hip_ctm", os.path.join(tmp, "out.ctm")])):
            tasks[name] = make_task(base + extra + ["--result_file", os.path.join(tmp, "result_%s.txt" % name)], conf)
            tasks[name][0].decode(tasks[name][1])  # warm-up: engine, workspace
        secs = {k: [] for k in tasks}
        for _ in range(a.cli_runs):
            for name, (task, targs) in tasks.items():
                secs[name].append(wall(lambda: task.decode(targs)))
        same = open(os.path.join(tmp, "result_plain.txt"), "rb").read() == open(os.path.join(tmp, "result_ctm.txt"), "rb").read()
        ctm_lines = sum(1 for _ in open(os.path.join(tmp, "out.ctm"), encoding="utf-8"))
        for task, _ in tasks.values():
            task.close()
    rec.update(cli_utterances=utts, cli_runs=a.cli_runs, result_files_identical=same, ctm_lines=ctm_lines,
               plain_loop_utt_per_sec=stats([utts / s for s in secs["plain"]], 1), plain_loop_with_ctm_utt_per_sec=stats([utts / s for s in secs["ctm"]], 1),
               with_ctm_over_plain=round(statistics.median(secs["plain"]) / statistics.median(secs["ctm"]), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--cli-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctc_times_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ctc_times: no GPU: nothing is measured without one")
    torch.set_num_threads(1)
    args = synth.make_args("config2")
    args.hip_precision, args.hip_max_batch, args.hip_max_frames = a.precision, a.batch, a.frames
    state = synth.make_state(args, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
    rec = {"workload": "bench workload: config 2, %d x %d frames, blank bias %.2f; greedy hypotheses as labels; legs taking turns in one "
                       "process, %d rounds; launches by HIP events (ProfScope), calls and the CLI by the host clock around a synchronise"
                       % (a.batch, a.frames, synth.BENCH_BLANK_BIAS, a.runs), "precision": a.precision}
    engine_legs(a, args, state, rec)
    cli_legs(a, synth.make_args("config2"), state, rec)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
