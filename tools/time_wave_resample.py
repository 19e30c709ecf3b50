"""decode_asr from a `wav.scp` at the front-end's rate, at 48 kHz stereo and at 8 kHz mono: the packed reader's wave form with and
without the resampling kernel in front of the fbank kernel, and against another checkout on the files both can read.

    python tools/time_wave_resample.py --workdir DIR --leg none                           # write the 16 kHz mono set once
    python tools/time_wave_resample.py --workdir DIR --leg 16k --out F.jsonl              # this tree: one timed decode per leg
    python tools/time_wave_resample.py --workdir DIR --leg 16k --package-root ab/parent --out F.jsonl   # the parent commit
    python tools/time_wave_resample.py --workdir DIR --leg 16k,48k2,8k --utts 2000 --out F.jsonl        # the new ground
    python tools/time_wave_resample.py --kernel                                           # one pass of 32 x 10 s, 48 kHz stereo
    python tools/time_wave_resample.py --summary F.jsonl

The ragged test set of tools/time_wave_reader.py's shape (--utts utterances of 300..1500 frames, same seed and lengths, the bench's
config-2 model and weights, a global CMVN stats file): one 16-bit WAV file per utterance, seeded Gaussian noise.  Leg `16k` holds it
as 16 kHz mono files - what every tree with audio input decodes; a tree with the resampler must take exactly its old path there (no
resampled pass is counted).  Leg `48k2` holds the same audio as 48 kHz stereo (every sample three times in channel 1, its negative
in channel 0; `--channel=1 --allow-downsample=true`), leg `8k` every second sample as 8 kHz mono (`--allow-upsample=true`): the
same frame counts (one less for some 8 kHz files), six times and half the bytes.  The sets of the new legs are written when a call
first asks for them.  Every leg is the default pipelined `decode_asr` (in process), `--hip_bucket 1`.

The two trees cannot share a process: call the tool once per tree and run, alternating, with the same --workdir; every call
appends one JSON line to --out.  --summary prints median and range per (tree, leg, utterances), whether the trees' result files
for a leg are the same, and for the 16 kHz leg whether the medians differ by no more than the other tree's own min-max spread.

--kernel runs Fbank.packed on one pass of 32 utterances of 10 s at 48 kHz stereo three times (for a kernel trace of its own:
rocprofv3 --kernel-trace --stats -- python tools/time_wave_resample.py --kernel) and prints the byte floor of the resampling
kernel: (2 C fi / fo + 4) bytes per output sample.
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
LEGS = {"16k": (16000, 1), "48k2": (48000, 2), "8k": (8000, 1)}
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak


def write_wav(path, x, rate, channels):
    data = np.ascontiguousarray(x, dtype="<i2").tobytes()
    head = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, 2 * channels * rate, 2 * channels, 16) + b"data" + struct.pack("<I", len(data))
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(head) + len(data)) + head + data)


def leg_audio(x, leg):
    """The 16 kHz samples ``x`` as the data chunk of leg ``leg``."""
    if leg == "16k":
        return x
    if leg == "8k":
        return x[::2]
    up = np.repeat(x, 3)
    return np.stack([-up - 1, up], axis=1).reshape(-1)  # (channel 0: another signal; -x - 1 stays inside int16)


def summary(path):
    runs, digests = {}, {}
    for line in open(path):
        rec = json.loads(line)
        for leg in rec.get("legs", []):
            runs.setdefault((rec["package_root"], leg, rec["utterances"]), []).extend(rec[leg]["utt_per_s"])
            digests.setdefault("%s:%d" % (leg, rec["utterances"]), set()).add(rec[leg]["result_sha1"])
    out = {"%s:%s:%d" % k: {"runs": len(v), "utt_per_s_median": statistics.median(v), "utt_per_s_min": min(v), "utt_per_s_max": max(v)}
           for k, v in sorted(runs.items())}
    out["result_files_identical_per_leg"] = {leg: len(d) == 1 for leg, d in digests.items()}
    trees = sorted(k for k in runs if k[1] == "16k")
    for k in trees:
        for other in trees:
            if other[0] != k[0] and other[2] == k[2] and k[0] == ".":
                spread = max(runs[other]) - min(runs[other])
                diff = statistics.median(runs[k]) - statistics.median(runs[other])
                out["16k:%d: this tree against %s" % (k[2], other[0])] = {
                    "median_difference_utt_per_s": round(diff, 1), "other_tree_min_max_spread": round(spread, 1),
                    "within_spread": bool(abs(diff) <= spread)}
    print(json.dumps(out), flush=True)
    return out


def kernel_pass(a):
    import torch

    from cassnat_asr_public_amd.data.fbank import Fbank

    rate, C, seconds, B = 48000, 2, 10, 32
    rng = np.random.default_rng(9)
    chunks = [np.ascontiguousarray(rng.integers(-20000, 20000, size=rate * seconds * C).astype("<i2")) for _ in range(B)]
    fb = Fbank(channel=1, allow_downsample=True)
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        feats, _ = fb.packed(chunks, rates=[rate] * B, channels=[C] * B)
        torch.cuda.synchronize()
        times.append(round(time.perf_counter() - t0, 5))
    outputs = B * seconds * 16000
    floor_bytes = (2 * C * rate / 16000 + 4) * outputs
    return {"kernel_pass": "32 x 10 s, 48 kHz stereo -> 16 kHz", "packed_seconds": times, "frames": int(feats.shape[1]), "output_samples": outputs,
            "resample_floor_bytes": int(floor_bytes), "resample_floor_us_at_8TBps": round(floor_bytes / HBM_BYTES_PER_S * 1e6, 2),
            "note": "wall time of Fbank.packed (gather, copy, launches, sync); the kernels' own times come from a kernel trace of this run"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--min-frames", type=int, default=300)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--runs", type=int, default=1, help="timed decodes per leg in this call")
    ap.add_argument("--leg", default="16k", help="comma list of 16k, 48k2, 8k; none: only write the 16 kHz set into --workdir")
    ap.add_argument("--workdir", default=None, help="where the test sets live (kept; default: a temporary directory)")
    ap.add_argument("--package-root", default=REPO, help="the checkout whose cassnat_asr_public_amd decodes")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    ap.add_argument("--kernel", action="store_true", help="one pass of 32 x 10 s at 48 kHz stereo through Fbank.packed instead")
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

    def emit(out):
        print(json.dumps(out), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(out) + "\n")

    if a.kernel:
        emit(kernel_pass(a))
        return
    margs = synth.make_args("config2")
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(a.min_frames, a.max_frames + 1, size=a.utts)]
    tmp_ctx = tempfile.TemporaryDirectory() if a.workdir is None else None
    work = a.workdir or tmp_ctx.name
    legs = [] if a.leg == "none" else a.leg.split(",")
    out = {}
    try:
        t0 = time.perf_counter()
        for leg in ["16k"] + [x for x in legs if x != "16k"]:
            rate, C = LEGS[leg]
            done = os.path.join(work, "written_%s_%d" % (leg, a.utts))
            if os.path.exists(done):
                continue
            os.makedirs(os.path.join(work, "wav_" + leg), exist_ok=True)
            with open(os.path.join(work, "%s_%d.scp" % (leg, a.utts)), "w") as f:
                for b, n in enumerate(lengths):
                    g = np.random.default_rng(4000 + b)
                    x = np.clip(np.rint(2000.0 * g.standard_normal(400 + 160 * (n - 1))), -32768, 32767).astype("<i2")
                    path = os.path.join(work, "wav_" + leg, f"spk-utt{b:05d}.wav")
                    write_wav(path, leg_audio(x, leg), rate, C)
                    f.write(f"spk-utt{b:05d} {path}\n")
            open(done, "w").close()
        if not os.path.exists(os.path.join(work, "model.mdl")):
            n = float(sum(lengths))  # Kaldi global CMVN stats (sums, sums of squares, count): features of about N(12, 3^2)
            stats = np.zeros((2, 81))
            stats[0, :-1], stats[0, -1], stats[1, :-1] = 12.0 * n, n, (3.0 ** 2 + 12.0 ** 2) * n
            kaldi_io.write_ark_scp(os.path.join(work, "cmvn.ark"), os.path.join(work, "cmvn.scp"), [("global", stats)])
            with open(os.path.join(work, "vocab.txt"), "w") as f:
                f.write("".join(f"w{i}\n" for i in range(margs.vocab_size - 4)))
            with open(os.path.join(work, "fbank.conf"), "w") as f:
                f.write("--allow-downsample=true\n--allow-upsample=true\n--channel=1\n")
            state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
            torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(work, "model.mdl"))
        out["setup_s"] = round(time.perf_counter() - t0, 1)
        keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
        conf = {k: getattr(margs, k) for k in keys}
        conf.update(vocab_file=os.path.join(work, "vocab.txt"), use_gpu=True, use_cmvn=True,
                    global_cmvn=kaldi_io.read_scp(os.path.join(work, "cmvn.scp"))[0][1])
        cfg = os.path.join(work, "decode.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump(conf, f)
        tag = hashlib.sha1(os.path.abspath(a.package_root).encode()).hexdigest()[:8]
        for leg in legs:
            scp = os.path.join(work, "%s_%d.scp" % (leg, a.utts))
            cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp, "--resume_model", os.path.join(work, "model.mdl"),
                   "--batch_size", str(a.batch), "--hip_precision", a.precision, "--hip_bucket", "1", "--hip_max_frames", str(a.max_frames),
                   "--print_freq", "100000", "--load_data_workers", "0", "--result_file", os.path.join(work, f"result_{leg}_{tag}.txt")]
            if leg != "16k":  # (the 16 kHz leg runs without a conf file: the command line a tree without the options takes too)
                cli += ["--hip_fbank_conf", os.path.join(work, "fbank.conf")]
            args = DecodeParser().get_args(cli)
            for k, v in conf.items():
                setattr(args, k, v)
            args.test_paths = [{"name": "test", "scp_path": scp}]
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
                rec.update(engine_passes=st["passes"], wave_passes=st.get("wave_passes", 0), resampled_passes=st.get("resampled_passes", 0))
            lines = open(args.result_file).read()
            assert len(lines.splitlines()) == a.utts
            assert rec["wave_passes"] == rec["engine_passes"] > 0, "the leg did not take the packed reader's wave form"
            assert rec["resampled_passes"] == (0 if leg == "16k" else rec["engine_passes"]), "resampled passes: %r" % rec
            rec["result_sha1"] = hashlib.sha1(lines.encode()).hexdigest()
            rec["bytes"] = sum(os.path.getsize(p) for _, p in kaldi_io.read_scp(scp))
            task.close()
            del task
            torch.cuda.empty_cache()
    finally:
        if tmp_ctx is not None:
            tmp_ctx.cleanup()
    out.update(utterances=a.utts, batch_size=a.batch, precision=a.precision, frames_min_max=[min(lengths), max(lengths)], legs=legs,
               package_root=os.path.relpath(os.path.abspath(a.package_root), REPO),
               note="default pipelined decode_asr, reading the files included; 48k2 / 8k: the 16 kHz samples repeated three times in "
                    "channel 1 of a stereo file / every second sample; profiler off")
    emit(out)


if __name__ == "__main__":
    main()
