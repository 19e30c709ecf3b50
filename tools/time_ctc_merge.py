"""Timing of the CTC prefix beam search that merges candidates by prefix (--hip_ctc_merge 1: cn_ctc_beam_merged) on the bench workload:
config 2, B utterances x 1000 frames, synth.BENCH_BLANK_BIAS, bf16 - the batch of tools/time_ctc_bias.py, 250 processed frames.  The
yardstick of every merged leg is the unmerged instantiation of the same policy in the same run.  Per ctc_beam / ctc_pruning setting:

  whole calls (encoder, CTC head, top-k, the search in one launch), six legs taking turns, `--runs` runs each (a run: `--inner` calls
  between two device synchronisations, the mean of them):
      none / none_merged    cn_ctc_beam / cn_ctc_beam_merged without a descriptor
      ngram / ngram_merged  cn_ctc_beam_ngram / cn_ctc_beam_merged with the synthetic order-3 ARPA model of tools/time_ctc_ngram.py
      bias / bias_merged    cn_ctc_beam_bias / cn_ctc_beam_merged with a 1000-phrase list (tools/time_ctc_bias.py's)
  the search kernel alone on the captured log-posteriors (cn_op_ctc_ngram_beam, cn_op_ctc_bias_beam, cn_op_ctc_merged_beam), where
  the stateless entries take the same pruned lists: ngram and bias, merged and not.

and, from the LM-free hypotheses: the number of distinct label sequences in the final unmerged beam against its width, and per
utterance the smallest merged beam at the same pruning whose best hypothesis equals the unmerged best of the widest setting, with the
merged search's time at the largest and at the median of those beams.  The synthetic model's posteriors are not speech: the last
figure shows the mechanism, not a word error rate.

One JSON line per setting, appended to --out (profiles/ctc_merge_time.jsonl).

    python tools/time_ctc_merge.py [--beams 5/8,20/30] [--batch 32] [--frames 1000] [--precision bf16] [--runs 5]
"""
import argparse
import ctypes as C
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
from cassnat_asr_public_amd.models.ngram import NgramLM, _ptr  # noqa: E402
from time_ctc_bias import random_phrases  # noqa: E402
from time_ctc_lm import load  # noqa: E402
from time_ctc_ngram import run_of  # noqa: E402
from time_esa import write_synthetic_arpa  # noqa: E402


def op_leg(L, name, head, dev, B, Tp, V, W, P, lp, with_scale):
    """A call of a stateless search entry on the captured log-posteriors; ``head``: the arguments in front of logp."""
    hyp = torch.empty(B, W, Tp + 1, dtype=torch.int32, device=dev.logp.device)
    hlen = torch.empty(B, W, dtype=torch.int32, device=dev.logp.device)
    sc, slm, pb, pnb = (torch.empty(B, W, dtype=torch.float64, device=dev.logp.device) for _ in range(4))
    nb = torch.empty(B, dtype=torch.int32, device=dev.logp.device)
    mid = (W, P, lp) + ((with_scale,) if with_scale is not None else ()) + (0,)
    fn = getattr(L, name)

    def call():
        hip.check(fn(*head, _ptr(dev.logp), _ptr(dev.top[P]), _ptr(dev.ratio), B, Tp, V, *mid, _ptr(hyp), Tp + 1, _ptr(hlen), _ptr(sc), _ptr(slm),
                     _ptr(pb), _ptr(pnb), _ptr(nb), hip.current_stream()))

    return call


def best_of(out):
    hyp, hlen = out[0].cpu().numpy(), out[1].cpu().numpy()
    return [tuple(hyp[b, 0, :hlen[b, 0]].tolist()) for b in range(hyp.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="5/8,20/30")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--lp", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--phrases", type=int, default=1000)
    ap.add_argument("--ngram-entries", type=int, default=1000000)
    ap.add_argument("--once", action="store_true", help="one call of every search kernel leg and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ctc_merge_time.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ctc_merge: no GPU: nothing is measured without one")
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
        write_synthetic_arpa(path, pieces, a.ngram_entries)
        ngram = NgramLM.load(path, vocab).cuda()
    ndesc = ngram.desc(ngram.device)
    opts = hip.Engine.make_opts(args)
    opts.sos = 1
    lm_scale = a.lm_weight * math.log(10.0)
    eng = model.engine(B, a.frames)
    settings = [tuple(int(x) for x in bp.split("/")) for bp in a.beams.split(",")]
    # the log-posteriors the searches run on, for the stateless entries
    copts = hip.Engine.make_opts(args, capture=True)
    copts.sos = 1
    hyp0, hlen0 = (t.cpu().numpy() for t in eng.ctc_beam(src, size, copts, settings[0][0], settings[0][1], a.lp)[:2])
    ctc = torch.from_numpy(np.ascontiguousarray(np.asarray(eng.fetch("ctc_out"), np.float32))).cuda()
    Tp = ctc.shape[1]
    dev = type("dev", (), dict(logp=ctc, ratio=size, top={P: torch.topk(ctc, P, dim=-1)[1].to(torch.int32).contiguous() for _, P in settings}))
    seen = [hyp0[b, 0, :3].tolist() for b in range(min(5, B)) if hlen0[b, 0] >= 3]
    bias = BiasList.from_phrases(random_phrases(a.phrases, V, a.phrases, seen)).cuda()
    bdesc = bias.desc(bias.device)
    L = eng.L
    widest = max(settings)
    best_wide = best_of(eng.ctc_beam(src, size, opts, widest[0], widest[1], a.lp))
    for W, P in settings:
        legs = {"none": lambda: eng.ctc_beam(src, size, opts, W, P, a.lp),
                "none_merged": lambda: eng.ctc_beam_merged(src, size, opts, W, P, a.lp),
                "ngram": lambda: eng.ctc_beam_ngram(ndesc, src, size, opts, W, P, a.lp, lm_scale),
                "ngram_merged": lambda: eng.ctc_beam_merged(src, size, opts, W, P, a.lp, ngram_desc=ndesc, lm_scale=lm_scale),
                "bias": lambda: eng.ctc_beam_bias(bdesc, src, size, opts, W, P, a.lp),
                "bias_merged": lambda: eng.ctc_beam_merged(src, size, opts, W, P, a.lp, bias_desc=bdesc)}
        ops = {"op_ngram": op_leg(L, "cn_op_ctc_ngram_beam", (C.byref(ndesc),), dev, B, Tp, V, W, P, a.lp, lm_scale),
               "op_ngram_merged": op_leg(L, "cn_op_ctc_merged_beam", (C.byref(ndesc), lm_scale, None), dev, B, Tp, V, W, P, a.lp, None),
               "op_bias": op_leg(L, "cn_op_ctc_bias_beam", (C.byref(bdesc),), dev, B, Tp, V, W, P, a.lp, None),
               "op_bias_merged": op_leg(L, "cn_op_ctc_merged_beam", (None, 0.0, C.byref(bdesc)), dev, B, Tp, V, W, P, a.lp, None),
               "op_none_merged": op_leg(L, "cn_op_ctc_merged_beam", (None, 0.0, None), dev, B, Tp, V, W, P, a.lp, None)}
        if a.once:
            for fn in list(ops.values()) + [legs["none"]]:
                fn()
            torch.cuda.synchronize()
            continue
        legs.update(ops)
        for fn in legs.values():  # warm-up of every leg at this shape
            fn()
        times = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fn in legs.items():
                times[k].append(run_of(fn, a.inner))
        med = {k: statistics.median(v) for k, v in times.items()}
        # what merging removes, and what a narrower merged beam finds (LM-free)
        plain = eng.ctc_beam(src, size, opts, W, P, a.lp)
        hyp, hlen, nb = (t.cpu().numpy() for t in (plain[0], plain[1], plain[5]))
        distinct = [len({tuple(hyp[b, j, :hlen[b, j]].tolist()) for j in range(int(nb[b]))}) for b in range(B)]
        merged = eng.ctc_beam_merged(src, size, opts, W, P, a.lp)
        mhyp, mhlen, mnb = (t.cpu().numpy() for t in (merged[0], merged[1], merged[6]))
        mdistinct = [len({tuple(mhyp[b, j, :mhlen[b, j]].tolist()) for j in range(int(mnb[b]))}) for b in range(B)]
        rec = {"workload": "bench workload: config 2, %d x %d frames (%d processed), blank bias %.2f; ctc_only, legs taking turns, %d runs each"
                           % (B, a.frames, Tp, synth.BENCH_BLANK_BIAS, a.runs),
               "precision": a.precision, "ctc_beam": W, "ctc_pruning": P, "phrases": len(bias.phrases),
               "unmerged_distinct_sequences_mean": round(float(np.mean(distinct)), 2), "unmerged_distinct_sequences_range": [min(distinct), max(distinct)],
               "unmerged_kept_mean": round(float(nb.mean()), 2), "merged_distinct_sequences_mean": round(float(np.mean(mdistinct)), 2),
               "merged_kept_mean": round(float(mnb.mean()), 2), "merged_best_equals_unmerged_best": int(sum(x == y for x, y in zip(best_of(merged), best_of(plain))))}
        for k in legs:
            rec[k + "_sec_per_batch_median"] = round(med[k], 6)
            rec[k + "_sec_per_batch_range"] = [round(min(times[k]), 6), round(max(times[k]), 6)]
        for k in ("none", "ngram", "bias", "op_ngram", "op_bias"):
            rec[k + "_merged_over_unmerged"] = round(med[k + "_merged"] / med[k], 3)
        if (W, P) == widest:
            # per utterance the smallest merged beam at this pruning whose best hypothesis is the unmerged best of this setting
            need = [None] * B
            for w in range(1, W + 1):
                got = best_of(eng.ctc_beam_merged(src, size, opts, w, P, a.lp))
                for b in range(B):
                    if need[b] is None and got[b] == best_wide[b]:
                        need[b] = w
            found = sorted(w for w in need if w is not None)
            rec["smallest_merged_beam_with_the_unmerged_best"] = need
            if found:
                for tag, w in (("largest", found[-1]), ("median", found[len(found) // 2])):
                    fn = lambda: eng.ctc_beam_merged(src, size, opts, w, P, a.lp)  # noqa: E731
                    fn()
                    t = [run_of(fn, a.inner) for _ in range(a.runs)]
                    rec["merged_beam_%s_needed" % tag] = w
                    rec["merged_beam_%s_needed_sec_per_batch_median" % tag] = round(statistics.median(t), 6)
                    rec["merged_beam_%s_needed_sec_per_batch_range" % tag] = [round(min(t), 6), round(max(t), 6)]
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
