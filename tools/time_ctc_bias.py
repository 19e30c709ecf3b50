"""Timing of the CTC prefix beam search with contextual phrase biasing (ctc_beam_decode with --hip_bias: cn_ctc_beam_bias) on the bench
workload: config 2, B utterances x 1000 frames, synth.BENCH_BLANK_BIAS, bf16 - the batch of tools/time_ctc_modes.py.  For every
ctc_beam / ctc_pruning setting and every phrase-list size (random phrases of 2-6 pieces over the config 2 vocabulary, score 3.0; five
phrases cut from the LM-free best hypotheses are on every list, so that phrases do complete; size 0 is the empty list, whose search
reads no table) three legs, alternating, `--runs` runs each (a run: `--inner` whole calls between two device synchronisations, the
mean of them), all in this process on this tree's library:

  bias    cn_ctc_beam_bias: encoder, CTC head, top-k, the biased search in one launch
  nolm    cn_ctc_beam at the same settings: the LM-free search
  ngram   cn_ctc_beam_ngram with the synthetic order-3 ARPA model of tools/time_ctc_ngram.py at the same settings

One JSON line per setting and list size: the median and the range of each leg in seconds per batch and the ratios of the medians.
Appended to --out (profiles/ctc_bias_time.jsonl).

    python tools/time_ctc_bias.py [--beams 5/8,20/30] [--lists 0,10,1000,5000] [--batch 32] [--frames 1000] [--precision bf16] [--runs 5]
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cassnat_asr_public_amd import hip, synth  # noqa: E402
from cassnat_asr_public_amd.models import make_cassnat_model  # noqa: E402
from cassnat_asr_public_amd.models.bias import BiasList  # noqa: E402
from cassnat_asr_public_amd.models.ngram import NgramLM  # noqa: E402
from time_ctc_lm import load  # noqa: E402
from time_ctc_ngram import run_of  # noqa: E402
from time_esa import write_synthetic_arpa  # noqa: E402


def random_phrases(n, V, seed, seen=()):
    rng = np.random.RandomState(seed)
    out = {tuple(p): 3.0 for p in seen}
    while len(out) < n:
        out[tuple(int(c) for c in rng.randint(4, V, rng.randint(2, 7)))] = 3.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="5/8,20/30")
    ap.add_argument("--lists", default="0,10,1000,5000")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--lp", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--ngram-entries", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ctc_bias_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ctc_bias: no GPU: nothing is measured without one")
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
    ndesc = ngram.desc(ngram.device)
    opts = hip.Engine.make_opts(args)
    opts.sos = 1
    lm_scale = a.lm_weight * math.log(10.0)
    eng = model.engine(B, a.frames)
    for W, P in ((int(x) for x in bp.split("/")) for bp in a.beams.split(",")):
        hyp, hlen = (t.cpu().numpy() for t in eng.ctc_beam(src, size, opts, W, P, a.lp)[:2])
        seen = [hyp[b, 0, k:k + 3].tolist() for b in range(5) for k in (0,) if hlen[b, 0] >= 3]
        for n in (int(x) for x in a.lists.split(",")):
            bias = BiasList.from_phrases(random_phrases(n, V, seed=n, seen=seen if n else ())).cuda()
            bdesc = bias.desc(bias.device)
            legs = {"bias": lambda: eng.ctc_beam_bias(bdesc, src, size, opts, W, P, a.lp),
                    "nolm": lambda: eng.ctc_beam(src, size, opts, W, P, a.lp),
                    "ngram": lambda: eng.ctc_beam_ngram(ndesc, src, size, opts, W, P, a.lp, lm_scale)}
            for fn in legs.values():  # warm-up of every leg at this shape
                fn()
            out = legs["bias"]()
            times = {k: [] for k in legs}
            for _ in range(a.runs):
                for k, fn in legs.items():
                    times[k].append(run_of(fn, a.inner))
            med = {k: statistics.median(v) for k, v in times.items()}
            rec = {"workload": "bench workload: config 2, %d x %d frames, blank bias %.2f; ctc_only, three legs alternating, %d runs each"
                               % (B, a.frames, synth.BENCH_BLANK_BIAS, a.runs),
                   "precision": a.precision, "ctc_beam": W, "ctc_pruning": P, "phrases": len(bias.phrases), "nodes": bias.nodes, "slots": bias.slots,
                   "table_bytes": int(bias.slots * 12 + bias.nodes * 13), "arpa_entries": entries,
                   "best_with_bonus": int((out[3][:, 0] != 0).sum()), "best_hyp_len_mean": round(float(out[1][:, 0].float().mean()), 1)}
            for k in legs:
                rec[k + "_sec_per_batch_median"] = round(med[k], 5)
                rec[k + "_sec_per_batch_range"] = [round(min(times[k]), 5), round(max(times[k]), 5)]
            rec["bias_over_nolm"] = round(med["bias"] / med["nolm"], 3)
            rec["ngram_over_nolm"] = round(med["ngram"] / med["nolm"], 3)
            rec["bias_and_nolm_ranges_overlap"] = bool(min(times["bias"]) <= max(times["nolm"]))
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
