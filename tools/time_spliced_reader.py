"""decode_asr with the recipes' feature configuration (left_ctx 0, right_ctx 2, skip_frame 1: input_size 240 from 80-dimensional
features) - the packed reader with the splice on the device against another checkout's path for the same set.

    python tools/time_spliced_reader.py --workdir DIR --leg none                    # write the test set once
    python tools/time_spliced_reader.py --workdir DIR --leg fm,cm,wav --out F.jsonl  # this tree: one timed decode per leg
    python tools/time_spliced_reader.py --workdir DIR --leg fm,cm --package-root ab/parent --out F.jsonl   # the parent commit
    python tools/time_spliced_reader.py --engine --out F.jsonl                       # the engine alone at input_size 240 and 80

The ragged test set of tools/time_compressed_reader.py (6000 utterances of 300..1500 frames, same seed and lengths, seeded N(0,1)
80-dimensional features, a global CMVN stats file) is written as an `FM ` archive, as the `CM` archive `copy-feats --compress=true`
would write (the `FM ` archive then holds ITS decompressed values, so the two legs decode the same numbers) and as one 16-bit WAV file
per utterance of the same frame counts (other values: the wave leg is reported alone).  The model is the bench's config-2 model at
input_size 240, seeded.  Every leg is the default pipelined `decode_asr` (in process), `--hip_bucket 1`, with `--hip_coalesce` as
given here: at this width the first convolution's image is about 1 GB per batch of 32 x 1000 frames.

A tree with the device splice takes the packed reader (one launch from the float32 staging buffer, two for compressed payloads and
samples); a tree without it takes the DataLoader's general host branch (CMVN in float64, np.vstack / np.hstack per utterance) and
cannot decode the wav.scp at all.  The two trees cannot share a process: call the tool once per tree and run, alternating, with the
same --workdir; every call appends one JSON line to --out (utt/s of each timed decode, the first call apart, the workers' host
seconds, which reader ran).  --summary F.jsonl prints median and range per (tree, leg) of the lines collected so far and checks
that every tree's result file for a leg is the same.
"""
import argparse
import hashlib
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_wav(path, x, rate=16000):
    data = np.ascontiguousarray(x, dtype="<i2").tobytes()
    head = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", len(data))
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(head) + len(data)) + head + data)


def summary(path):
    runs, digests = {}, {}
    for line in open(path):
        rec = json.loads(line)
        for leg in rec.get("legs", []):
            key = (rec["package_root"], leg)
            runs.setdefault(key, []).extend(rec[leg]["utt_per_s"])
            digests.setdefault(leg, set()).add(rec[leg]["result_sha1"])
    out = {"%s:%s" % k: {"runs": len(v), "utt_per_s_median": statistics.median(v), "utt_per_s_min": min(v), "utt_per_s_max": max(v)}
           for k, v in sorted(runs.items())}
    out["result_files_identical_per_leg"] = {leg: len(d) == 1 for leg, d in digests.items()}
    print(json.dumps(out), flush=True)
    return out


def engine_alone(a):
    """The engine without a reader: 32 x 1000-frame device-resident batches through two decode pipelines (what bench.py times), at
    input_size 240 and at 80."""
    import torch

    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.models.cassnat import make_model
    from cassnat_asr_public_amd.pipeline import DecodePipelines

    out = {}
    for width in (240, 80):
        args = synth.make_args("config2", input_size=width, n_features=80, right_ctx=(width // 80 - 1))
        args.hip_precision, args.hip_max_batch, args.hip_max_frames = a.precision, a.batch, 1000
        model = make_model(width, args).cuda()
        state = synth.make_state(args, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
        with torch.no_grad():
            for k, p in model.named_parameters():
                p.copy_(torch.from_numpy(state[k]))
        fh, sh = synth.make_feats(a.batch, 1000, width, seed=1234)
        feats, sizes = torch.from_numpy(fh).cuda(), torch.from_numpy(sh).cuda()
        pipes = DecodePipelines(model, 2, a.batch, 1000, coalesce=a.coalesce)

        def run(n):
            for _ in pipes.decode([(feats, sizes, k) for k in range(n)], args, sos=1, as_lists=False):
                pass
            torch.cuda.synchronize()

        run(a.coalesce * 4)
        rates = []
        for _ in range(5):
            t0 = time.perf_counter()
            run(a.steps)
            rates.append(round(a.steps * a.batch / (time.perf_counter() - t0), 1))
        pipes.close()
        del model, pipes
        torch.cuda.empty_cache()
        out["input_size_%d" % width] = {"utt_per_s": rates, "utt_per_s_median": statistics.median(rates)}
    out.update(mode="engine", precision=a.precision, batch_size=a.batch, frames=1000, steps=a.steps, coalesce=a.coalesce, pipelines=2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--min-frames", type=int, default=300)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--right-ctx", type=int, default=2)
    ap.add_argument("--coalesce", type=int, default=4, help="--hip_coalesce of every leg")
    ap.add_argument("--runs", type=int, default=1, help="timed decodes per leg in this call")
    ap.add_argument("--leg", default="fm,cm,wav", help="comma list of fm, cm, wav; none: only write the test set into --workdir")
    ap.add_argument("--workdir", default=None, help="where the test set lives (kept; default: a temporary directory)")
    ap.add_argument("--package-root", default=REPO, help="the checkout whose cassnat_asr_public_amd decodes")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    ap.add_argument("--engine", action="store_true", help="time the engine alone at input_size 240 and 80 instead")
    ap.add_argument("--steps", type=int, default=40, help="--engine: batches per timed run")
    ap.add_argument("--summary", default=None, help="print median and range per (tree, leg) of this JSONL file and exit")
    a = ap.parse_args()
    if a.summary:
        summary(a.summary)
        return
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    import yaml

    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.data import kaldi_io
    from cassnat_asr_public_amd.tasks import CassNATTask
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    torch.set_num_threads(1)
    if a.engine:
        out = engine_alone(a)
        print(json.dumps(out), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(out) + "\n")
        return
    blocks = a.right_ctx + 1
    margs = synth.make_args("config2", input_size=80 * blocks, n_features=80, right_ctx=a.right_ctx)
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(a.min_frames, a.max_frames + 1, size=a.utts)]
    tmp_ctx = tempfile.TemporaryDirectory() if a.workdir is None else None
    work = a.workdir or tmp_ctx.name
    os.makedirs(os.path.join(work, "wav"), exist_ok=True)
    out = {}
    try:
        scp = {k: os.path.join(work, k + ".scp") for k in ("cm", "fm", "wav")}
        done = os.path.join(work, "written_%d" % a.utts)
        t0 = time.perf_counter()
        if not os.path.exists(done):
            def mats():
                for b, n in enumerate(lengths):
                    f, _ = synth.make_feats(1, n, 80, seed=4000 + b)
                    yield f"spk-utt{b:05d}", f[0]

            kaldi_io.write_ark_scp(os.path.join(work, "cm.ark"), scp["cm"], mats(), compress=1)
            kaldi_io.write_ark_scp(os.path.join(work, "fm.ark"), scp["fm"], ((u, kaldi_io.load_mat(s)) for u, s in kaldi_io.read_scp(scp["cm"])))
            with open(scp["wav"], "w") as f:
                for b, n in enumerate(lengths):
                    g = np.random.default_rng(4000 + b)
                    path = os.path.join(work, "wav", f"spk-utt{b:05d}.wav")
                    write_wav(path, np.clip(np.rint(2000.0 * g.standard_normal(400 + 160 * (n - 1))), -32768, 32767))
                    f.write(f"spk-utt{b:05d} {path}\n")
            n = float(sum(lengths))  # Kaldi global CMVN stats (sums, sums of squares, count) of N(0.2, 1.5^2) features
            stats = np.zeros((2, 81))
            stats[0, :-1], stats[0, -1], stats[1, :-1] = 0.2 * n, n, (1.5 ** 2 + 0.2 ** 2) * n
            kaldi_io.write_ark_scp(os.path.join(work, "cmvn.ark"), os.path.join(work, "cmvn.scp"), [("global", stats)])
            with open(os.path.join(work, "vocab.txt"), "w") as f:
                f.write("".join(f"w{i}\n" for i in range(margs.vocab_size - 4)))
            state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
            torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(work, "model.mdl"))
            open(done, "w").close()
        out["setup_s"] = round(time.perf_counter() - t0, 1)
        keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
        conf = {k: getattr(margs, k) for k in keys}
        conf.update(vocab_file=os.path.join(work, "vocab.txt"), use_gpu=True, use_cmvn=True,
                    global_cmvn=kaldi_io.read_scp(os.path.join(work, "cmvn.scp"))[0][1])
        cfg = os.path.join(work, "decode.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump(conf, f)
        legs = [] if a.leg == "none" else a.leg.split(",")
        tag = hashlib.sha1(os.path.abspath(a.package_root).encode()).hexdigest()[:8]
        for leg in legs:
            cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp[leg], "--resume_model", os.path.join(work, "model.mdl"),
                   "--batch_size", str(a.batch), "--hip_precision", a.precision, "--hip_bucket", "1", "--hip_max_frames", str(a.max_frames),
                   "--hip_coalesce", str(a.coalesce), "--print_freq", "100000", "--load_data_workers", "0",
                   "--result_file", os.path.join(work, f"result_{leg}_{tag}.txt")]
            args = DecodeParser().get_args(cli)
            for k, v in conf.items():
                setattr(args, k, v)
            args.test_paths = [{"name": "test", "scp_path": scp[leg]}]
            args.rank = 0
            task = CassNATTask("test", args)
            task.load_lm_model(args)
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            task.decode(args)  # the first call creates engines, workspaces, threads and the row-count predictor
            torch.cuda.synchronize()
            rec = out[leg] = {"first_call_seconds": round(time.perf_counter() - c0, 3), "seconds": [], "utt_per_s": [], "worker_host_seconds": []}
            for _ in range(max(1, a.runs)):
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                task.decode(args)
                torch.cuda.synchronize()
                el = time.perf_counter() - c0
                st = task.pipeline_stats
                rec["seconds"].append(round(el, 4))
                rec["utt_per_s"].append(round(a.utts / el, 1))
                rec["worker_host_seconds"].append({k: round(v, 3) for k, v in st.items() if k.startswith("s_")})
                rec.update(engine_passes=st["passes"], spliced_passes=st.get("spliced_passes", 0),
                           compressed_passes=st.get("compressed_passes", 0), wave_passes=st.get("wave_passes", 0))
            lines = open(args.result_file).read()
            assert len(lines.splitlines()) == a.utts
            rec["result_sha1"] = hashlib.sha1(lines.encode()).hexdigest()
            task.close()
            del task
            torch.cuda.empty_cache()
    finally:
        if tmp_ctx is not None:
            tmp_ctx.cleanup()
    out.update(utterances=a.utts, batch_size=a.batch, precision=a.precision, frames_min_max=[min(lengths), max(lengths)], legs=legs,
               right_ctx=a.right_ctx, input_size=80 * blocks, hip_coalesce=a.coalesce,
               package_root=os.path.relpath(os.path.abspath(a.package_root), REPO),
               note="default pipelined decode_asr, reading the set included; fm = the float32 archive of the CM archive's decompressed values")
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
