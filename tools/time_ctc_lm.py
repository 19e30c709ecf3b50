"""Timing of the CTC prefix beam search with the TransformerLM in the frame loop (ctc_beam_decode with ctc_lm_weight > 0:
cn_ctc_beam_lm) on the bench workload: config 2, B utterances x 1000 frames, synth.BENCH_BLANK_BIAS, bf16.  One JSON line per
(LM preset, ctc_beam / ctc_pruning):

  sec_per_batch / utt_per_sec   the whole cn_ctc_beam_lm call (encoder, CTC head, top-k, schedule, the loop, the unroll)
  iterations                    iterations of the loop = the largest number of processed frames of an utterance
  nolm_sec_per_batch            cn_ctc_beam at the same beam / pruning: the encoder pass and the LM-free search
  ms_per_iteration              (sec_per_batch - nolm_sec_per_batch) / iterations: the loop without the encoder pass (the LM-free
                                search's own kernel, a few ms per batch, is subtracted with it)
  ms_per_iteration_whole_call   sec_per_batch / iterations: nothing subtracted
  lm_ms_per_step                the bare cn_lm_step loop over the same number of slots with pos = the iteration index (identity
                                ancestor table: every row reads pos + 1 keys, an upper bound on the search's key counts), timed in the
                                same process, alternating with the fused call
  loop_over_lm                  ms_per_iteration / lm_ms_per_step (the aim of DESIGN 7d: <= 1.25 for lm_recipe at 20 / 30)

If the LM handle refuses the slots of the full batch the batch is halved until it fits, and the line says which batch ran.

    python tools/time_ctc_lm.py [--lm lm_small,lm_recipe] [--beams 5/8,20/30] [--batch 32] [--frames 1000] [--precision bf16] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cassnat_asr_public_amd import hip, synth  # noqa: E402
from cassnat_asr_public_amd.models import make_cassnat_model  # noqa: E402
from cassnat_asr_public_amd.models.lm import make_model as make_lm  # noqa: E402


def load(model, state):
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[k]))
    return model


def timed(fn, reps):
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return min(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lm", default="lm_small,lm_recipe")
    ap.add_argument("--beams", default="5/8,20/30")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--lp", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    args = synth.make_args("config2", decode_type="ctc_only", ctc_lm_weight=a.lm_weight, ctc_lp=a.lp)
    args.hip_precision, args.hip_max_batch, args.hip_max_frames = a.precision, a.batch, a.frames
    model = load(make_cassnat_model(args.input_size, args).cuda(), synth.make_state(args, seed=0, blank_bias=synth.BENCH_BLANK_BIAS))
    feats, sizes = synth.make_feats(a.batch, a.frames, args.input_size, seed=1234)
    src_all, size_all = torch.from_numpy(feats).cuda(), torch.from_numpy(sizes).cuda()
    V = args.vocab_size
    opts = hip.Engine.make_opts(args)
    opts.sos = 1
    for preset in a.lm.split(","):
        lm_args = synth.make_args_lm(preset, vocab_size=V)
        lm_args.hip_precision = a.precision
        lm = load(make_lm(lm_args).cuda(), synth.make_state(lm_args, seed=9))
        for W, P in ((int(x) for x in bp.split("/")) for bp in a.beams.split(",")):
            B = a.batch
            while True:
                src, size = src_all[:B].contiguous(), size_all[:B].contiguous()
                eng = model.engine(B, a.frames)
                S = B * W
                try:
                    lm_eng = lm.step_engine(S)
                    iters = eng.ctc_beam_lm(lm_eng, src, size, opts, W, P, a.lp, a.lm_weight)[-1]
                    break
                except hip.HipError as e:
                    if B == 1:
                        raise
                    print(json.dumps({"refused": str(e), "batch": B, "lm": preset, "ctc_beam": W}), flush=True)
                    B //= 2
            tok = torch.full((S,), 5, dtype=torch.int32, device="cuda")
            anc = torch.arange(S, dtype=torch.int32, device="cuda").view(S, 1).repeat(1, iters + 1).contiguous()
            keyok = torch.ones(S, iters + 1, dtype=torch.uint8, device="cuda")
            logp = torch.empty(S, V, dtype=torch.float32, device="cuda")

            def fused():
                eng.ctc_beam_lm(lm_eng, src, size, opts, W, P, a.lp, a.lm_weight)

            def bare():
                for pos in range(iters):
                    lm_eng.lm_step(pos, tok, anc, keyok, logp)

            def nolm():
                eng.ctc_beam(src, size, opts, W, P, a.lp)

            ft, lt, nt = [], [], []
            for _ in range(a.reps):
                ft.append(timed(fused, 1))
                lt.append(timed(bare, 1))
                nt.append(timed(nolm, 1))
            whole, bare_t, nolm_t = min(ft), min(lt), min(nt)
            loop = whole - nolm_t
            print(json.dumps({
                "workload": "bench workload: config 2, %d x %d frames, blank bias %.2f; CTC prefix beam search + LM in the loop" % (B, a.frames, synth.BENCH_BLANK_BIAS),
                "lm": preset, "lm_weight": a.lm_weight, "ctc_beam": W, "ctc_pruning": P, "slots": S, "precision": a.precision,
                "sec_per_batch": round(whole, 4), "utt_per_sec": round(B / whole, 2), "iterations": iters,
                "nolm_sec_per_batch": round(nolm_t, 4), "ms_per_iteration": round(1e3 * loop / iters, 3),
                "ms_per_iteration_whole_call": round(1e3 * whole / iters, 3), "lm_ms_per_step": round(1e3 * bare_t / iters, 3),
                "loop_over_lm": round(loop / bare_t, 3), "whole_call_over_lm": round(whole / bare_t, 3),
                "fused_sec_spread": [round(x, 4) for x in sorted(ft)], "lm_sec_spread": [round(x, 4) for x in sorted(lt)]}), flush=True)


if __name__ == "__main__":
    main()
