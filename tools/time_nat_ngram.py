"""Timing of CASS-NAT decoding with word n-gram fusion in the finish loop (CassNAT.beam_decode with lm_weight > 0 and an NgramLM:
cn_nat_ngram_finish) on the bench workload: config 2, B utterances x 1000 frames, synth.BENCH_BLANK_BIAS, bf16, the synthetic order-3
ARPA model of tools/time_ctc_ngram.py.  For every beam width three legs take turns in one process, `--runs` timed whole beam_decode
calls each after a warm-up:

  ngram   the n-gram finish (decode pass that keeps its rows, class tables, the finish launch, the host's records)
  nolm    lm_weight 0: the greedy finish at beam 1, the host beam over the fetched top-k tables above it
  lm      the TransformerLM finish with `--lm` (lm_small)

`nolm` and `lm` run code this change does not touch: they are the yardstick.  One JSON line per beam width, appended to --out
(profiles/nat_ngram_time.jsonl): median and range of every leg in seconds per batch, utt/s of the medians, whether the n-gram leg's
range lies wholly below the lm leg's, whether its utt/s is above the nolm leg's; and, from HIP events around the two new launches
(cn_profile_begin) over `--runs` further calls, their milliseconds per batch and the class top-k's bytes per second beside the
B * U * V * 4 bytes it must read.

    python tools/time_nat_ngram.py [--beam 1,5,10] [--batch 32] [--frames 1000] [--precision bf16] [--runs 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cassnat_asr_public_amd import synth  # noqa: E402
from cassnat_asr_public_amd.models import make_cassnat_model  # noqa: E402
from cassnat_asr_public_amd.models.lm import make_model as make_lm  # noqa: E402
from cassnat_asr_public_amd.models.ngram import NgramLM  # noqa: E402
from time_ctc_lm import load  # noqa: E402
from time_esa import write_synthetic_arpa  # noqa: E402


def run_of(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beam", default="1,5,10")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--lm", default="lm_small")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ngram-entries", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nat_ngram_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_nat_ngram: no GPU: nothing is measured without one")
    args = synth.make_args("config2", length_penalty=0)
    args.hip_precision, args.hip_max_batch, args.hip_max_frames = a.precision, a.batch, a.frames
    model = load(make_cassnat_model(args.input_size, args).cuda(), synth.make_state(args, seed=0, blank_bias=synth.BENCH_BLANK_BIAS))
    feats, sizes = synth.make_feats(a.batch, a.frames, args.input_size, seed=1234)
    src, size = torch.from_numpy(feats).cuda(), torch.from_numpy(sizes).cuda()
    B, V = a.batch, args.vocab_size
    pieces = ["blank", "sos", "eos", "unk"] + [("p%d" if i % 4 == 3 else "▁p%d") % i for i in range(4, V)]
    vocab = type("vocab", (), dict(index2word=dict(enumerate(pieces)), word2index={p: i for i, p in enumerate(pieces)}, n_words=V))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "synthetic.arpa")
        entries = write_synthetic_arpa(path, pieces, a.ngram_entries)
        ngram = NgramLM.load(path, vocab).cuda()
    lm_args = synth.make_args_lm(a.lm, vocab_size=V)
    lm_args.hip_precision = a.precision
    lm = load(make_lm(lm_args).cuda(), synth.make_state(lm_args, seed=9))

    def leg(lm_weight, rank, lm_model):
        def fn():
            args.lm_weight, args.rank_model = lm_weight, rank
            return model.beam_decode(src, None, size, vocab, args, lm_model)[0]
        return fn

    for bw in (int(x) for x in a.beam.split(",")):
        args.beam_width = bw
        legs = {"ngram": leg(a.lm_weight, "n-gram", ngram), "nolm": leg(0, "lm", None), "lm": leg(a.lm_weight, "lm", lm)}
        outs = {k: fn() for k, fn in legs.items()}  # warm-up of every leg at this beam
        times = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fn in legs.items():
                times[k].append(run_of(fn))
        eng = model._engine
        legs["ngram"]()
        U = int(eng.shape("tok")[1])
        eng.profile_begin(["nat_class_topk", "nat_ngram_finish"])
        for _ in range(a.runs):
            legs["ngram"]()
        prof = eng.profile_end()
        med = {k: statistics.median(v) for k, v in times.items()}
        topk_ms = prof["nat_class_topk"]["ms"] / prof["nat_class_topk"]["count"]
        rec = {"workload": "bench workload: config 2, %d x %d frames, blank bias %.2f; whole beam_decode calls, three legs taking turns, "
                           "%d runs each" % (B, a.frames, synth.BENCH_BLANK_BIAS, a.runs),
               "precision": a.precision, "beam_width": bw, "lm_weight": a.lm_weight, "arpa_entries": entries, "arpa_order": ngram.order, "lm_leg": a.lm,
               "finish_steps": U, "best_differs_from_nolm": sum(x[0]["hyp"] != y[0]["hyp"] for x, y in zip(outs["ngram"], outs["nolm"]))}
        for k in legs:
            rec[k + "_sec_per_batch_median"] = round(med[k], 5)
            rec[k + "_sec_per_batch_range"] = [round(min(times[k]), 5), round(max(times[k]), 5)]
            rec[k + "_utt_per_sec"] = round(B / med[k], 1)
        rec["ngram_range_wholly_below_lm"] = bool(max(times["ngram"]) < min(times["lm"]))
        rec["ngram_utt_per_sec_above_nolm"] = bool(med["ngram"] < med["nolm"])
        rec["class_topk_ms_per_batch"] = round(topk_ms, 4)
        rec["ngram_finish_ms_per_batch"] = round(prof["nat_ngram_finish"]["ms"] / prof["nat_ngram_finish"]["count"], 4)
        rec["class_topk_row_bytes"] = B * U * V * 4
        rec["class_topk_gb_per_sec"] = round(B * U * V * 4 / (topk_ms * 1e-3) / 1e9, 1)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
