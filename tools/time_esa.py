"""Timing of ESA decoding (sample_num alignments per utterance + TransformerLM ranking: the shipped cassnat_decode.yaml's
mode) on the bench shape: config 2 model, B utterances x 1000 frames, LM preset lm_small.  Not the headline bench; prints
one JSON line.
    python tools/time_esa.py [--batch 32] [--frames 1000] [--samples 50] [--precision bf16]
`--rank n-gram` ranks with models.ngram.NgramLM over a synthetic ARPA file (orders 1-3, about 1e6 entries over the config 2
vocabulary, written to a temporary directory) and also times the ranking step alone: on the device, and through the host loop of
CassNAT._esa_decode (one Python string and one score(text) call per sample) on the same token rows."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cassnat_asr_public_amd import synth  # noqa: E402
from cassnat_asr_public_amd.models.cassnat import make_model  # noqa: E402
from cassnat_asr_public_amd.models.lm import make_model as make_lm  # noqa: E402


class Vocab:
    word2index = {"blank": 0, "sos": 1, "eos": 2, "unk": 3}


def write_synthetic_arpa(path, pieces, entries=1000000, seed=0):
    """A closed order-3 ARPA text over the one-piece words of `pieces`: every word a 1-gram, about 30 % of the rest 2-grams, the
    others 3-grams (a, b, c) put together from two 2-grams (a, b), (b, c)."""
    rng = np.random.RandomState(seed)
    words = sorted({p.replace("\u2581", "") for p in pieces} - {""})
    uni = ["<unk>", "<s>", "</s>"] + words
    n = len(uni)
    n2 = max(1, int(0.3 * (entries - n)))
    a = rng.randint(0, n, 2 * n2)
    b = rng.randint(0, n, 2 * n2)
    ok = (a != 2) & (b != 1)  # nothing follows </s>, <s> follows nothing
    pairs = np.unique(a[ok].astype(np.int64) * n + b[ok])[:n2]
    rng.shuffle(pairs)
    pa, pb = pairs // n, pairs % n
    order = np.argsort(pa, kind="stable")
    first = np.searchsorted(pa[order], np.arange(n))           # the 2-grams that begin with word w: order[first[w] : first[w + 1]]
    count = np.diff(np.append(first, len(pairs)))
    n3 = max(1, entries - n - len(pairs))
    pick = rng.randint(0, len(pairs), 2 * n3)
    pick = pick[count[pb[pick]] > 0]
    nxt = order[first[pb[pick]] + (rng.randint(0, 1 << 30, len(pick)) % count[pb[pick]])]
    tri = np.unique((pa[pick] * n + pb[pick]) * n + pb[nxt])[:n3]
    prob = lambda k: -rng.uniform(0.05, 4.0, k)  # noqa: E731
    lines = ["\\data\\", "ngram 1=%d" % n, "ngram 2=%d" % len(pairs), "ngram 3=%d" % len(tri), "", "\\1-grams:"]
    lines += ["%.4f\t%s\t%.4f" % (p, w, q) for p, w, q in zip(prob(n), uni, -rng.uniform(0, 1.5, n))]
    lines += ["", "\\2-grams:"]
    lines += ["%.4f\t%s %s\t%.4f" % (p, uni[x], uni[y], q) for p, x, y, q in zip(prob(len(pairs)), pa, pb, -rng.uniform(0, 1.5, len(pairs)))]
    lines += ["", "\\3-grams:"]
    lines += ["%.4f\t%s %s %s" % (p, uni[x], uni[y], uni[z]) for p, x, y, z in zip(prob(len(tri)), tri // (n * n), tri // n % n, tri % n)]
    lines += ["", "\\end\\", ""]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines))
    return n + len(pairs) + len(tri)


def time_ngram_rank_alone(lm, vocab, tok, ylen, reps=3):
    """The ranking step on token rows a decode produced: the device path, and the host loop of CassNAT._esa_decode."""
    dev, host = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = lm.score_tokens(tok, ylen).cpu()
        dev.append(time.perf_counter() - t0)
    for _ in range(reps):
        t0 = time.perf_counter()
        tok_c, n_c = tok.cpu().numpy(), ylen.cpu().numpy()
        ref = [lm.score("".join(vocab.index2word[int(t)] for t in row[:n] if int(t) != 2).replace("\u2581", " ").strip()) for row, n in zip(tok_c, n_c)]
        host.append(time.perf_counter() - t0)
    assert np.array_equal(sc.numpy().view(np.int32), np.array(ref, np.float32).view(np.int32)), "device and host ranking disagree"
    return min(dev[1:]), min(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--same-seed", action="store_true", help="the same random draws in every repetition")
    ap.add_argument("--rank", default="lm", choices=["lm", "at_baseline", "n-gram"],
                    help="ranker: the TransformerLM (lm_small), the autoregressive baseline (config 4 model, teacher-forced) or an "
                         "ARPA n-gram model (synthetic, orders 1-3, --ngram-entries entries)")
    ap.add_argument("--ngram-entries", type=int, default=1000000)
    ap.add_argument("--group", type=int, default=0, help="args.hip_esa_group: samples per decoder-side pass (0: the package's default)")
    a = ap.parse_args()
    args = synth.make_args("config2", sample_num=a.samples, rank_model=a.rank, threshold=0.9)
    if a.group > 0:
        args.hip_esa_group = a.group
    args.hip_precision = a.precision
    args.hip_max_batch, args.hip_max_frames = a.batch, a.frames
    extra, vocab, rows = {}, Vocab, []
    state = synth.make_state(args, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
    model = make_model(args.input_size, args).cuda()
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(state[k]))
    if a.rank == "n-gram":
        from cassnat_asr_public_amd.models.ngram import NgramLM

        class vocab(Vocab):  # three pieces in four begin a word, the fourth continues one
            index2word = dict(enumerate(["blank", "sos", "eos", "unk"] + [("p%d" if i % 4 == 3 else "\u2581p%d") % i for i in range(4, args.vocab_size)]))
            n_words = args.vocab_size

        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "synthetic.arpa")
            extra["arpa_entries"] = write_synthetic_arpa(path, list(vocab.index2word.values()), a.ngram_entries)
            extra["arpa_mbytes"] = round(os.path.getsize(path) / 1e6, 1)
            t0 = time.perf_counter()
            lm = NgramLM.load(path, vocab).cuda()
            torch.cuda.synchronize()
            extra["arpa_load_sec"] = round(time.perf_counter() - t0, 3)
        extra["arpa_unclosed"] = lm.unclosed
        rank_on_device = lm.score_tokens  # (keep the rows the decode hands to the ranker: they are timed alone below)
        lm.score_tokens = lambda tok, ylen, drop_id=2: (rows.append((tok, ylen)), rank_on_device(tok, ylen, drop_id))[1]
    else:
        if a.rank == "lm":
            lm_args = synth.make_args_lm("lm_small", vocab_size=args.vocab_size)
        else:
            lm_args = synth.make_args_ast("config4", vocab_size=args.vocab_size)
        lm_args.hip_precision = a.precision
        lm_state = synth.make_state(lm_args, seed=9, gain=2.0)
        if a.rank == "lm":
            lm = make_lm(lm_args).cuda()
        else:
            from cassnat_asr_public_amd.models.transformer import make_model as make_ast

            lm = make_ast(lm_args.input_size, lm_args).cuda()
        with torch.no_grad():
            for k, p in lm.named_parameters():
                p.copy_(torch.from_numpy(lm_state[k]))
    fh, sh = synth.make_feats(a.batch, a.frames, args.input_size, seed=1234)
    src, sizes = torch.from_numpy(fh).cuda(), torch.from_numpy(sh).cuda()
    mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    times = []
    for r in range(a.reps + 1):
        torch.manual_seed(0 if a.same_seed else r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, _ = model.beam_decode(src, mask, sizes, vocab, args, lm)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    best = min(times[1:])
    if a.rank == "n-gram":
        lm.score_tokens = rank_on_device
        dev_s, host_s = time_ngram_rank_alone(lm, vocab, *rows[-1])
        extra.update(rank_device_ms=round(dev_s * 1e3, 3), rank_host_loop_ms=round(host_s * 1e3, 1), rank_rows=int(rows[-1][0].shape[0]),
                     rank_stride=int(rows[-1][0].shape[1]))
    ranker = {"lm": "TransformerLM lm_small", "at_baseline": "autoregressive-baseline (config 4 model)", "n-gram": "ARPA n-gram (synthetic, order 3)"}[a.rank]
    print(json.dumps({"workload": f"ESA: config 2 model, sample_num {a.samples}, " + ranker + " ranking", **extra,
                      "batch": a.batch, "frames": a.frames, "precision": a.precision, "esa_group": a.group or None, "sec_per_batch": round(best, 4),
                      "utt_per_sec": round(a.batch / best, 2), "rtf": round(best / (a.batch * a.frames * 0.01), 6),
                      "tokens_max": max(len(o[0]["hyp"]) for o in out) - 1, "all_runs_sec": [round(t, 4) for t in times]}))


if __name__ == "__main__":
    main()
