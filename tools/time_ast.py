"""Timing of the autoregressive (AST) path at BASELINE configs[3] shape: same 12-layer encoder, 6 decoder layers, beam 10,
ctc_beam 15, joint CTC/attention scoring; B utterances x 1000 frames.  Not the headline bench (bench.py measures
configs[1]); prints one JSON line with utterances/s, ms per decode step and where a step's wall time goes.
``--model conformer``: the conformer AST (models/conformer.py, synth preset config4_conf) - the same decoder (6 layers, d_decff
2048, now Swish) behind a 12-layer conformer encoder.  Both models report the encoder pass (cn_ast_begin: encoder, cross K|V, CTC
preparation) apart from the decoder steps: ``decoder_ms_per_step`` = (search - encoder) / steps.

``--lm lm_small|lm_recipe``: LM shallow fusion (transformer.py:186-209) with a seeded TransformerLM of that synth preset
(lm_recipe = conf/lm.yaml: 16 layers, d 512); ``lm_ms_per_step`` times the LM step alone (cn_lm_step over the same slots and
positions).  ``--beam`` / ``--ctc-beam``: run_art.sh stage 3 uses 20 / 30.
``--lm ngram``: word n-gram shallow fusion (include/cassnat_hip_ast_ngram.h) with a synthetic order-3 ARPA model of about
``--ngram-entries`` entries (time_esa.write_synthetic_arpa) over a vocabulary of one-piece words and continuation pieces.
``--alternate none,ngram,lm_recipe --rounds 5``: the legs named take turns in one process, ``--rounds`` timed decodes each (after
one warm-up each); one JSON line per leg with the median and the range of ms per step and utt/s, and nothing else is measured.
A leg ``biasN`` (``bias10``, ``bias5000``) decodes with a synthetic phrase list of N phrases (include/cassnat_hip_ast_bias.h; its
``ngram_entries`` field holds N); with ``--ctc-weight 0`` its fused top-K kernel runs in place of the terms kernel.

    python tools/time_ast.py [--model transformer|conformer] [--batch 32] [--frames 1000] [--precision bf16] [--ctc-weight 0.3] [--ratio 0.3]
                             [--lm none|lm_small|lm_recipe|ngram] [--lm-weight 0.6] [--beam 10] [--ctc-beam 15] [--ngram-entries N]
                             [--alternate none,ngram,lm_recipe --rounds 5]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cassnat_asr_public_amd import hip, synth  # noqa: E402
from cassnat_asr_public_amd.models.conformer import make_model as make_conformer  # noqa: E402
from cassnat_asr_public_amd.models.lm import make_model as make_lm  # noqa: E402
from cassnat_asr_public_amd.models.transformer import make_model as make_transformer  # noqa: E402


class Vocab:
    word2index = {"blank": 0, "sos": 1, "eos": 2, "unk": 3}


def piece_vocab(n):
    """A vocabulary of n pieces for the n-gram legs: the four specials, then three one-piece words for every continuation piece."""
    pieces = ["blank", "sos", "eos", "unk"] + [("c%d" if i % 4 == 3 else "\u2581w%d") % i for i in range(n - 4)]
    v = Vocab()
    v.index2word, v.n_words = dict(enumerate(pieces)), n
    return v


def make_ngram(vocab, entries):
    from cassnat_asr_public_amd.models.ngram import NgramLM
    from time_esa import write_synthetic_arpa

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "synthetic.arpa")
        n = write_synthetic_arpa(path, [vocab.index2word[i] for i in range(4, vocab.n_words)], entries=entries)
        lm = NgramLM.load(path, vocab).cuda()
    return lm, n


def make_bias(vocab_size, phrases, seed=5):
    """A synthetic phrase list for the ``biasN`` legs: N phrases of 1 to 4 random pieces (no special id), scores 0.5 .. 3."""
    import numpy as np

    from cassnat_asr_public_amd.models.bias import BiasList

    rng = np.random.RandomState(seed)
    out = {}
    while len(out) < phrases:
        out[tuple(int(t) for t in rng.randint(4, vocab_size, rng.randint(1, 5)))] = float(rng.choice([0.5, 1.0, 2.0, 3.0]))
    return BiasList.from_phrases(out).cuda()


def make_transformer_lm(preset, vocab_size, precision):
    lm_args = synth.make_args_lm(preset, vocab_size=vocab_size)
    lm_args.hip_precision = precision
    lm = make_lm(lm_args).cuda()
    lm_state = synth.make_state(lm_args, seed=9)
    with torch.no_grad():
        for k, p in lm.named_parameters():
            p.copy_(torch.from_numpy(lm_state[k]))
    return lm


def alternate(a, args, model, src, mask):
    """The legs of --alternate in turn, --rounds times: per leg the median and range of ms per decode step and utt/s."""
    vocab = piece_vocab(args.vocab_size)
    legs = {}
    for name in a.alternate.split(","):
        largs = copy.copy(args)
        largs.lm_weight = 0 if name == "none" or name.startswith("bias") else a.lm_weight
        entries, bias = None, None
        if name == "none":
            lm = None
        elif name.startswith("bias"):  # (biasN: a list of N phrases, include/cassnat_hip_ast_bias.h)
            lm, entries = None, int(name[4:])
            bias = make_bias(args.vocab_size, entries)
        elif name == "ngram":
            lm, entries = make_ngram(vocab, a.ngram_entries)
        else:
            lm = make_transformer_lm(name, args.vocab_size, a.precision)
        legs[name] = dict(args=largs, lm=lm, bias=bias, entries=entries, sec=[], steps=0)
    for r in range(a.rounds + 1):  # (round 0 warms every leg up)
        for name, leg in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            beams = model.beam_decode(src, mask, vocab, leg["args"], leg["lm"], bias=leg["bias"])
            torch.cuda.synchronize()
            if r:
                leg["sec"].append(time.perf_counter() - t0)
            leg["steps"] = max(len(b[0]["hyp"]) for b in beams) - 1
    for name, leg in legs.items():
        ms = [1e3 * t / max(leg["steps"], 1) for t in leg["sec"]]
        ups = [a.batch / t for t in leg["sec"]]
        print(json.dumps({"leg": name, "model": a.model, "precision": a.precision, "batch": a.batch, "frames": a.frames, "beam": a.beam,
                          "ctc_beam": a.ctc_beam, "ctc_weight": a.ctc_weight, "lm_weight": leg["args"].lm_weight, "ngram_entries": leg["entries"],
                          "rounds": a.rounds, "decode_steps": leg["steps"],
                          "ms_per_decode_step": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
                          "utt_per_sec": {"median": round(statistics.median(ups), 2), "min": round(min(ups), 2), "max": round(max(ups), 2)},
                          "all_runs_sec": [round(t, 4) for t in leg["sec"]]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("transformer", "conformer"), default="transformer")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--ratio", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--streams", type=int, default=1,
                    help="decode pipelines (engine handle + HIP stream + host thread each) working on independent batches: a decode "
                         "step occupies a handful of CUs, so throughput - not latency - scales with pipelines")
    ap.add_argument("--lm", choices=("none", "lm_small", "lm_recipe", "ngram"), default="none")
    ap.add_argument("--ngram-entries", type=int, default=1000000)
    ap.add_argument("--alternate", default="", help="comma-separated legs (none, ngram, biasN, lm_small, lm_recipe) that take turns in one process")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lm-weight", type=float, default=0.6)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--ctc-beam", type=int, default=15)
    a = ap.parse_args()
    args = synth.make_args_ast("config4" if a.model == "transformer" else "config4_conf", ctc_weight=a.ctc_weight,
                               max_decode_ratio=a.ratio, beam_width=a.beam, ctc_beam=a.ctc_beam,
                               lm_weight=a.lm_weight if a.lm != "none" else 0)
    make_model = make_transformer if a.model == "transformer" else make_conformer
    args.hip_precision = a.precision
    args.hip_max_batch = a.batch
    args.hip_max_frames = a.frames
    state = synth.make_state(args, seed=0, gain=2.0)
    feats, _ = synth.make_feats(a.batch, a.frames, args.input_size, seed=1234)
    model = make_model(args.input_size, args).cuda()
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[k]))
    src = torch.from_numpy(feats).cuda()
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    if a.alternate:
        return alternate(a, args, model, src, mask)
    lm, vocab, ngram_entries = None, Vocab, None
    if a.lm == "ngram":
        vocab = piece_vocab(args.vocab_size)
        lm, ngram_entries = make_ngram(vocab, a.ngram_entries)
    elif a.lm != "none":
        lm = make_transformer_lm(a.lm, args.vocab_size, a.precision)
    times = []
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        beams = model.beam_decode(src, mask, vocab, args, lm)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    steps = max(len(b[0]["hyp"]) for b in beams) - 1
    # the encoder pass alone, on the same handle and workspace
    eng = model.engine(a.batch, a.frames)
    opts = hip.CnDecodeOpts(padding_idx=int(args.padding_idx), sos=1, beam_width=1)
    use_ctc = a.ctc_weight > 0
    enc = []
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ast_begin(src, opts, use_ctc, steps + 1, a.batch * int(args.beam_width), int(args.ctc_beam) if use_ctc else 0)
        torch.cuda.synchronize()
        enc.append(time.perf_counter() - t0)
    enc_best = min(enc[1:])
    lm_ms = None
    if lm is not None and a.lm != "ngram":  # the LM step alone on the beam's slots, position after position (identity ancestor table)
        S = a.batch * int(args.beam_width)
        leng = lm.step_engine(S)
        leng.lm_step_begin(steps + 1, S)
        tok = torch.full((S,), 5, dtype=torch.int32, device="cuda")
        anc = torch.arange(S, dtype=torch.int32, device="cuda").view(S, 1).repeat(1, steps + 1).contiguous()
        keyok = torch.ones(S, steps + 1, dtype=torch.uint8, device="cuda")
        logp = torch.empty(S, args.vocab_size, dtype=torch.float32, device="cuda")
        lt = []
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for pos in range(steps):
                leng.lm_step(pos, tok, anc, keyok, logp)
            torch.cuda.synchronize()
            lt.append(time.perf_counter() - t0)
        lm_ms = round(1e3 * min(lt[1:]) / max(steps, 1), 3)
    out = {"workload": "BASELINE configs[3]: AST beam search, 12L enc / 6L dec, beam %d, ctc_beam %d" % (args.beam_width, args.ctc_beam),
           "lm": a.lm, "lm_weight": args.lm_weight, "lm_ms_per_step": lm_ms, "ngram_entries": ngram_entries,
           "model": a.model, "encoder": "conformer (d_encff 1024, kernel 31, max_rel 20)" if a.model == "conformer" else "transformer",
           "decoder_ffn": "swish" if a.model == "conformer" else "relu",
           "encoder_ms": round(1e3 * enc_best, 3), "decoder_ms_per_step": round(1e3 * (best - enc_best) / max(steps, 1), 3),
           "batch": a.batch, "frames": a.frames, "precision": a.precision, "ctc_weight": a.ctc_weight,
           "decode_steps": steps, "sec_per_batch": round(best, 4), "utt_per_sec": round(a.batch / best, 2),
           "rtf": round(best / (a.batch * a.frames * 0.01), 6), "ms_per_decode_step": round(1e3 * best / max(steps, 1), 3),
           "all_runs_sec": [round(t, 4) for t in times]}
    if a.streams > 1:
        import threading

        models = [model]
        for _ in range(a.streams - 1):
            m2 = make_model(args.input_size, args).cuda()
            with torch.no_grad():
                for k, p in m2.named_parameters():
                    p.copy_(torch.from_numpy(state[k]))
            models.append(m2)
        S = a.batch * int(args.beam_width)  # one LM handle (own step cache) per pipeline, one copy of the LM weights
        lm_engs = [None] * a.streams if lm is None or a.lm == "ngram" else [lm.step_engine(S)] + [lm.new_engine(S, share=lm.step_engine(S))
                                                                                 for _ in range(a.streams - 1)]

        def worker(i, n):
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(n):
                    models[i].beam_decode(src, mask, vocab, args, lm, lm_engine=lm_engs[i])
                st.synchronize()

        for n in (1, a.reps):  # warm-up round (engine builds), then the timed one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            th = [threading.Thread(target=worker, args=(i, n)) for i in range(a.streams)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
        out.update({"pipelines": a.streams, "pipelined_utt_per_sec": round(a.streams * a.reps * a.batch / el, 2),
                    "pipelined_sec_per_batch": round(el / (a.streams * a.reps), 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
