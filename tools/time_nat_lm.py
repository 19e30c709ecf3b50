"""Timing of CASS-NAT decoding with LM shallow fusion (CassNAT.beam_decode with lm_weight > 0: the finish loop on the device,
cn_nat_lm_finish) on the bench workload: config 2, B utterances x 1000 frames, synth.BENCH_BLANK_BIAS, bf16.  One JSON line per
(LM preset, beam width):

  sec_per_batch / utt_per_sec   the whole beam_decode call (decode pass + fused finish + the host's records)
  finish_steps                  steps of the finish loop (the pass's row count)
  ms_per_finish_step            cn_nat_lm_finish alone on the rows the pass left, per step
  lm_ms_per_step                the bare cn_lm_step loop over the same slots and positions (identity ancestor table), timed in the
                                same process, alternating with the fused loop: the floor of a finish step
  nolm_sec_per_batch            the same beam width with lm_weight 0 (decode pass + host beam over the fetched top-k), for context

    python tools/time_nat_lm.py [--lm lm_small,lm_recipe] [--beam 1,5,10] [--batch 32] [--frames 1000] [--precision bf16] [--reps 3]
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


class Vocab:
    word2index = {"blank": 0, "sos": 1, "eos": 2, "unk": 3}


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
    ap.add_argument("--beam", default="1,5,10")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    args = synth.make_args("config2", length_penalty=0)
    args.hip_precision, args.hip_max_batch, args.hip_max_frames = a.precision, a.batch, a.frames
    model = load(make_cassnat_model(args.input_size, args).cuda(), synth.make_state(args, seed=0, blank_bias=synth.BENCH_BLANK_BIAS))
    feats, sizes = synth.make_feats(a.batch, a.frames, args.input_size, seed=1234)
    src, size = torch.from_numpy(feats).cuda(), torch.from_numpy(sizes).cuda()
    B, V = a.batch, args.vocab_size
    for preset in a.lm.split(","):
        lm_args = synth.make_args_lm(preset, vocab_size=V)
        lm_args.hip_precision = a.precision
        lm = load(make_lm(lm_args).cuda(), synth.make_state(lm_args, seed=9))
        for bw in (int(x) for x in a.beam.split(",")):
            args.beam_width = bw
            args.lm_weight = 0
            nolm = timed(lambda: model.beam_decode(src, None, size, Vocab, args, None), a.reps)
            args.lm_weight = a.lm_weight
            whole = timed(lambda: model.beam_decode(src, None, size, Vocab, args, lm), a.reps)
            # the finish alone, on the rows the last pass left in the engine, alternating with the bare LM step loop
            eng = model._engine
            steps = int(eng.shape("tok")[1])
            S = B * bw
            opts = hip.Engine.make_opts(args)
            lm_eng = lm.step_engine(S)
            lm_eng.lm_step_begin(steps + 1, S)
            hyp = torch.empty(B, bw, steps + 1, dtype=torch.int32, device="cuda")
            hyp_len = torch.empty(B, bw, dtype=torch.int32, device="cuda")
            score = torch.empty(B, bw, dtype=torch.float64, device="cuda")
            tok = torch.full((S,), 5, dtype=torch.int32, device="cuda")
            anc = torch.arange(S, dtype=torch.int32, device="cuda").view(S, 1).repeat(1, steps + 1).contiguous()
            keyok = torch.ones(S, steps + 1, dtype=torch.uint8, device="cuda")
            logp = torch.empty(S, V, dtype=torch.float32, device="cuda")
            eng.nat_attach_lm(lm_eng)

            def fused():
                eng.nat_lm_finish(opts, steps, bw, args.lm_weight, args.length_penalty, False, hyp, hyp_len, score)

            def bare():
                for pos in range(steps):
                    lm_eng.lm_step(pos, tok, anc, keyok, logp)

            ft, lt = [], []
            for _ in range(a.reps):
                ft.append(timed(fused, 1))
                lt.append(timed(bare, 1))
            eng.nat_attach_lm(None)
            fin, bare_t = min(ft), min(lt)
            print(json.dumps({
                "workload": "bench workload: config 2, %d x %d frames, blank bias %.2f; CASS-NAT + LM finish on the device" % (B, a.frames, synth.BENCH_BLANK_BIAS),
                "lm": preset, "lm_weight": a.lm_weight, "beam_width": bw, "slots": S, "precision": a.precision,
                "sec_per_batch": round(whole, 4), "utt_per_sec": round(B / whole, 2), "finish_steps": steps,
                "ms_per_finish_step": round(1e3 * fin / steps, 3), "lm_ms_per_step": round(1e3 * bare_t / steps, 3),
                "finish_over_lm": round(fin / bare_t, 3), "finish_sec": round(fin, 4),
                "nolm_sec_per_batch": round(nolm, 4), "nolm_utt_per_sec": round(B / nolm, 2)}), flush=True)


if __name__ == "__main__":
    main()
