"""Timing of the CTC prefix beam search with word n-gram fusion (ctc_beam_decode with an NgramLM: cn_ctc_beam_ngram) on the bench
workload: config 2, B utterances x 1000 frames, synth.BENCH_BLANK_BIAS, bf16, a synthetic order-3 ARPA model of the size
tools/time_esa.py --rank n-gram uses (about 1e6 entries over the config 2 vocabulary; three pieces in four begin a word).  For every
ctc_beam / ctc_pruning setting three legs, alternating, `--runs` runs each (a run: `--inner` whole calls between two device
synchronisations, the mean of them), all in this process on this tree's library:

  ngram   cn_ctc_beam_ngram: encoder, CTC head, top-k, the n-gram search in one launch
  nolm    cn_ctc_beam at the same settings: the LM-free search
  lm      cn_ctc_beam_lm with the TransformerLM `--lm` (lm_small) at the same settings

One JSON line per setting: the median and the range of each leg in seconds per batch, the ratios of the medians, and whether the
ranges of `ngram` and `lm` overlap.  Appended to --out (profiles/ctc_ngram_time.jsonl).

    python tools/time_ctc_ngram.py [--beams 5/8,20/30] [--batch 32] [--frames 1000] [--precision bf16] [--runs 5] [--once 5/8]

`--once W/P` runs one n-gram batch at that setting after a warm-up and exits: the command to put behind rocprofv3 --kernel-trace.
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cassnat_asr_public_amd import hip, synth  # noqa: E402
from cassnat_asr_public_amd.models import make_cassnat_model  # noqa: E402
from cassnat_asr_public_amd.models.lm import make_model as make_lm  # noqa: E402
from cassnat_asr_public_amd.models.ngram import NgramLM  # noqa: E402
from time_ctc_lm import load  # noqa: E402
from time_esa import write_synthetic_arpa  # noqa: E402


def run_of(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="5/8,20/30")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--lm", default="lm_small")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--lp", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--ngram-entries", type=int, default=1000000)
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ctc_ngram_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ctc_ngram: no GPU: nothing is measured without one")
    args = synth.make_args("config2", decode_type="ctc_only", ctc_lm_weight=a.lm_weight, ctc_lp=a.lp)
    args.hip_precision, args.hip_max_batch, args.hip_max_frames = a.precision, a.batch, a.frames
    model = load(make_cassnat_model(args.input_size, args).cuda(), synth.make_state(args, seed=0, blank_bias=synth.BENCH_BLANK_BIAS))
    feats, sizes = synth.make_feats(a.batch, a.frames, args.input_size, seed=1234)
    src, size = torch.from_numpy(feats).cuda().contiguous(), torch.from_numpy(sizes).cuda().contiguous()
    V, B = args.vocab_size, a.batch
    pieces = ["blank", "sos", "eos", "unk"] + [("p%d" if i % 4 == 3 else "▁p%d") % i for i in range(4, V)]
    vocab = type("vocab", (), dict(index2word=dict(enumerate(pieces)), n_words=V))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "synthetic.arpa")
        entries = write_synthetic_arpa(path, pieces, a.ngram_entries)
        ngram = NgramLM.load(path, vocab).cuda()
    desc = ngram.desc(ngram.device)
    opts = hip.Engine.make_opts(args)
    opts.sos = 1
    lm_scale = a.lm_weight * math.log(10.0)
    eng = model.engine(B, a.frames)
    if a.once:
        W, P = (int(x) for x in a.once.split("/"))
        for _ in range(2):
            out = eng.ctc_beam_ngram(desc, src, size, opts, W, P, a.lp, lm_scale)
            torch.cuda.synchronize()
        print(json.dumps({"once": a.once, "hyp_len_best_mean": float(out[1][:, 0].float().mean())}))
        return
    lm_args = synth.make_args_lm(a.lm, vocab_size=V)
    lm_args.hip_precision = a.precision
    lm = load(make_lm(lm_args).cuda(), synth.make_state(lm_args, seed=9))
    for W, P in ((int(x) for x in bp.split("/")) for bp in a.beams.split(",")):
        lm_eng = lm.step_engine(B * W)
        legs = {"ngram": lambda: eng.ctc_beam_ngram(desc, src, size, opts, W, P, a.lp, lm_scale),
                "nolm": lambda: eng.ctc_beam(src, size, opts, W, P, a.lp),
                "lm": lambda: eng.ctc_beam_lm(lm_eng, src, size, opts, W, P, a.lp, a.lm_weight)}
        inner = {"ngram": a.inner, "nolm": a.inner, "lm": 1}
        out = legs["ngram"]()
        for fn in legs.values():  # warm-up of every leg at this shape
            fn()
        iters = legs["lm"]()[-1]
        times = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fn in legs.items():
                times[k].append(run_of(fn, inner[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"workload": "bench workload: config 2, %d x %d frames, blank bias %.2f; ctc_only, three legs alternating, %d runs each"
                           % (B, a.frames, synth.BENCH_BLANK_BIAS, a.runs),
               "precision": a.precision, "ctc_beam": W, "ctc_pruning": P, "lm_weight": a.lm_weight, "arpa_entries": entries, "arpa_order": ngram.order,
               "lm_leg": a.lm, "processed_frames_max": iters, "best_hyp_len_mean": round(float(out[1][:, 0].float().mean()), 1)}
        for k in legs:
            rec[k + "_sec_per_batch_median"] = round(med[k], 5)
            rec[k + "_sec_per_batch_range"] = [round(min(times[k]), 5), round(max(times[k]), 5)]
        rec["ngram_over_nolm"] = round(med["ngram"] / med["nolm"], 3)
        rec["lm_over_ngram"] = round(med["lm"] / med["ngram"], 2)
        rec["ngram_and_lm_ranges_overlap"] = bool(max(times["ngram"]) >= min(times["lm"]))
        rec["ngram_below_lm"] = bool(med["ngram"] < med["lm"])
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
