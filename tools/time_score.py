"""Timing of the scorer (cn_op_edit_align, decode_asr --hip_score).  All legs run in one process and take turns, `--runs` rounds after a
warm-up; medians and ranges by the host clock around work that ends in a device synchronise.  One JSON line, appended to --out
(profiles/score_time.jsonl):

  1. two synthetic sets of --pairs pairs at 10 % errors - word-like (10 .. 60 units a side) and token-like (100 .. 700) - through
     ``hip.edit_align`` with the copies to and from the device, through the entry alone on resident buffers (the launch and the drain
     of the stream), through the serial host entry ``hip.edit_align_host``, and - on the first --model-pairs pairs, once - through the
     pure-Python model of the tests (tests/edit_model.py); the outputs of the legs are compared;
  2. decode_asr (pipelined, in process) on the ragged synthetic list of tools/ragged_cli_bench.py (--utts utterances of 300 .. 1500
     frames) with and without --hip_score, the reference being the run's own result file with 10 % of its pieces changed.

    python tools/time_score.py [--pairs 3000] [--runs 5] [--utts 6000] [--precision bf16]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import edit_model  # noqa: E402
from cassnat_asr_public_amd import hip, synth  # noqa: E402
from cassnat_asr_public_amd.data import kaldi_io  # noqa: E402
from ragged_cli_bench import make_task  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "range": [round(min(xs), digits), round(max(xs), digits)]}


def noisy(rng, ref, alphabet, rate):
    """``ref`` with about ``rate`` of its units deleted, replaced or followed by an inserted one (a third each)."""
    out = []
    for x in ref:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(int(rng.integers(alphabet)) if u < 2 * rate / 3 else x)
        if u > 1 - rate / 3:
            out.append(int(rng.integers(alphabet)))
    return out


def pair_set(seed, pairs, lo, hi, alphabet):
    rng = np.random.default_rng(seed)
    refs = [rng.integers(alphabet, size=int(rng.integers(lo, hi + 1))).tolist() for _ in range(pairs)]
    hyps = [noisy(rng, r, alphabet, 0.10) for r in refs]
    rl, hl = np.array([len(r) for r in refs], np.int32), np.array([len(h) for h in hyps], np.int32)
    return {"refs": refs, "hyps": hyps, "ref": np.array([x for r in refs for x in r], np.int32), "hyp": np.array([x for h in hyps for x in h], np.int32),
            "rl": rl, "hl": hl, "rb": np.cumsum(rl, dtype=np.int64) - rl, "hb": np.cumsum(hl, dtype=np.int64) - hl}


def op_legs(a, name, s):
    keys = ("ref", "rb", "rl", "hyp", "hb", "hl")
    mr, mh = int(s["rl"].max()), int(s["hl"].max())
    res = [t.cuda() for t in map(torch.from_numpy, (s[k] for k in keys))]
    got = {}

    def with_copies():
        out = hip.edit_align(*(torch.from_numpy(s[k]).cuda() for k in keys), max_ref=mr, max_hyp=mh)
        got["dev"] = [t.cpu().numpy() for t in out]

    def resident():
        got["res"] = hip.edit_align(*res, max_ref=mr, max_hyp=mh)

    def host():
        got["host"] = hip.edit_align_host(*(s[k] for k in keys), max_ref=mr, max_hyp=mh)

    legs = {"op_with_copies_ms": with_copies, "op_resident_ms": resident, "host_entry_ms": host}
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, fn in legs.items():
            ms[k].append(wall(fn) * 1e3)
    same = all(np.array_equal(x, y) for x, y in zip(got["dev"], got["host"]))
    m = min(a.model_pairs, len(s["refs"]))
    t0 = time.perf_counter()
    model = [edit_model.align(s["refs"][n], s["hyps"][n]) for n in range(m)]
    model_ms = (time.perf_counter() - t0) * 1e3
    cost, _, plen, ops, ob = got["host"]
    same = same and all(model[n][0] == cost[n] and model[n][1] == ops[ob[n]:ob[n] + plen[n]].tolist() for n in range(m))
    counts = got["host"][1].sum(0)
    rec = {"pairs": len(s["refs"]), "units_per_side": [int(min(s["rl"].min(), s["hl"].min())), int(max(mr, mh))], "cells": int((s["rl"].astype(np.int64) * s["hl"]).sum()),
           "error_rate_percent": round(100.0 * float(counts[1:].sum()) / float(counts[:3].sum()), 2),
           "outputs_identical": bool(same), "model_pairs": m, "model_ms": round(model_ms, 1), "model_ms_per_pair": round(model_ms / m, 4)}
    for k in legs:
        rec[k] = stats(ms[k])
        rec[k.replace("_ms", "_us_per_pair")] = round(1e3 * statistics.median(ms[k]) / len(s["refs"]), 3)
    rec["host_entry_over_op_with_copies"] = round(statistics.median(ms["host_entry_ms"]) / statistics.median(ms["op_with_copies_ms"]), 3)
    return {name: rec}


def cli_legs(a, rec):
    margs = synth.make_args("config2")
    state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(300, 1501, size=a.utts)]
    with tempfile.TemporaryDirectory() as tmp:
        def mats():
            for b, n in enumerate(lengths):
                f, _ = synth.make_feats(1, n, margs.input_size, seed=4000 + b)
                yield "spk-utt%05d" % b, f[0]

        scp = os.path.join(tmp, "feats.scp")
        kaldi_io.write_ark_scp(os.path.join(tmp, "feats.ark"), scp, mats())
        with open(os.path.join(tmp, "utt2num_frames"), "w") as f:
            f.write("".join("spk-utt%05d %d\n" % (b, n) for b, n in enumerate(lengths)))
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
        base = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", ckpt, "--batch_size", "32", "--hip_precision", a.precision,
                "--hip_bucket", "1", "--hip_max_frames", "1500", "--print_freq", "100000", "--load_data_workers", "0"]
        ref_file, out_dir = os.path.join(tmp, "token.scp"), os.path.join(tmp, "score")
        tasks = {"plain": make_task(base + ["--result_file", os.path.join(tmp, "result_plain.txt")], conf)}
        tasks["plain"][0].decode(tasks["plain"][1])  # warm-up: engines, workspaces, threads; its result file gives the reference
        pieces = ["w%d" % i for i in range(margs.vocab_size - 4)]
        units = 0
        with open(ref_file, "w") as f:
            for line in open(os.path.join(tmp, "result_plain.txt")):
                utt, hyp = line.split()[0], line.split()[1:]
                ref = [pieces[x] if isinstance(x, int) else x for x in noisy(rng, hyp, len(pieces), 0.10)]
                units += len(ref)
                f.write(" ".join([utt] + ref) + "\n")
        tasks["score"] = make_task(base + ["--result_file", os.path.join(tmp, "result_score.txt"), "--hip_score", out_dir, "--hip_score_ref", ref_file], conf)
        tasks["score"][0].decode(tasks["score"][1])
        secs = {k: [] for k in tasks}
        for _ in range(a.runs):
            for name, (task, targs) in tasks.items():
                secs[name].append(wall(lambda: task.decode(targs)))
        same = open(os.path.join(tmp, "result_plain.txt"), "rb").read() == open(os.path.join(tmp, "result_score.txt"), "rb").read()
        wer = open(os.path.join(out_dir, "wer")).read().splitlines()
        for task, _ in tasks.values():
            task.close()
    rec["decode_asr"] = {"utterances": a.utts, "frames_min_max": [min(lengths), max(lengths)], "reference_units": units, "result_files_identical": same,
                         "wer_line": wer[0], "unit_line": wer[3], "plain_seconds": stats(secs["plain"]), "with_score_seconds": stats(secs["score"]),
                         "score_seconds_added": round(statistics.median(secs["score"]) - statistics.median(secs["plain"]), 3),
                         "with_score_over_plain": round(statistics.median(secs["score"]) / statistics.median(secs["plain"]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--model-pairs", type=int, default=30)
    ap.add_argument("--utts", type=int, default=6000, help="0: no decode_asr leg")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_score: no GPU: nothing is measured without one")
    torch.set_num_threads(1)
    rec = {"workload": "synthetic pairs at 10 %% errors (a third each deleted, replaced, inserted), costs 1/1/1; legs taking turns in one process, %d "
                       "rounds after a warm-up, host clock around a synchronise" % a.runs}
    rec.update(op_legs(a, "word_like", pair_set(11, a.pairs, 10, 60, 20000)))
    rec.update(op_legs(a, "token_like", pair_set(12, a.pairs, 100, 700, 5000)))
    if a.utts:
        cli_legs(a, rec)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
