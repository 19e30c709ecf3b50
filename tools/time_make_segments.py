"""bin/make_segments on a synthetic set of long recordings, device leg against host-twin leg, and decode_asr --hip_segments on one
long recording beside decode_asr on a wav.scp of separately written files that hold the same sample ranges.

    python tools/time_make_segments.py [--minutes 10,20,30,60] [--runs 5] [--decode-runs 5] [--decode-minutes 10]
                                       [--out profiles/make_segments_time.jsonl] [--workdir DIR]

The recordings are 16 kHz mono: bursts of modulated noise at speech level (1 .. 8 s) between stretches of +-3 noise (0.3 .. 2 s), seeded.
Legs, taking turns in one process, --runs times each after a first call (buffers, page-locked memory, the files into the page cache):
    device   --hip_vad device: frame energies and the decision by the kernels
    host     --hip_vad host: the serial twins of the same tree (the baseline: the parent commit has no tool)
Every run reads the files and writes segments, vad.scp and vad.ark; both legs must write the same bytes.  Then the segments of the
first --decode-minutes recording are decoded twice with the bench's config-2 weights (bf16): in place (--hip_segments) and from
pre-cut WAV files of exactly the samples [first, last), alternating --decode-runs times.
Prints one JSON line (and appends it to --out): recordings/s and seconds of audio per second per leg (every run, median, range), the
decode seconds of both forms, their ratio and spread.

--only LEG: that one leg once, nothing else - the run to put under `rocprofv3 --kernel-trace --stats` (on its own: a profiler changes
the timings of everything else); the energy kernel's byte floor is the staged bytes (printed) over the HBM bandwidth."""
import argparse
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
    body = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, rate * 2, 2, 16) + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def recording(minutes, seed, rate=16000):
    rng = np.random.default_rng(seed)
    n, parts, at = int(minutes * 60 * rate), [], 0
    while at < n:
        quiet = int(rng.uniform(0.3, 2.0) * rate)
        burst = int(rng.uniform(1.0, 8.0) * rate)
        parts.append(rng.integers(-3, 4, quiet).astype(np.int16))
        env = 0.55 + 0.45 * np.sin(np.arange(burst) * (2 * np.pi * rng.uniform(2.0, 5.0) / rate))
        parts.append(np.clip(rng.standard_normal(burst) * 3000.0 * env, -32768, 32767).astype(np.int16))
        at += quiet + burst
    return np.concatenate(parts)[:n]


def median_range(xs):
    return {"median": statistics.median(xs), "range": [min(xs), max(xs)], "all": xs}


def read_dir(path):
    return {n: open(os.path.join(path, n), "rb").read() for n in sorted(os.listdir(path))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", default="10,20,30,60")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--decode-runs", type=int, default=5, help="0: no decode comparison")
    ap.add_argument("--decode-minutes", type=float, default=10)
    ap.add_argument("--decode-batch", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--only", default=None, choices=["device", "host"], help="run that leg once and stop (for a profiler)")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    import yaml

    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.bin import make_segments as ms
    from cassnat_asr_public_amd.data import segments
    from cassnat_asr_public_amd.tasks import CassNATTask
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    torch.set_num_threads(1)
    minutes = [float(m) for m in a.minutes.split(",")]
    tmp_ctx = tempfile.TemporaryDirectory() if a.workdir is None else None
    work = a.workdir or tmp_ctx.name
    os.makedirs(work, exist_ok=True)
    out = {}
    try:
        t0 = time.perf_counter()
        scp = os.path.join(work, "wav.scp")
        with open(scp, "w") as f:
            for k, m in enumerate(minutes):
                path = os.path.join(work, "rec%02d.wav" % k)
                if not os.path.exists(path):
                    write_wav(path, recording(m, 900 + k))
                f.write("rec%02d %s\n" % (k, path))
        audio_s = 60.0 * sum(minutes)
        out.update(setup_s=round(time.perf_counter() - t0, 1), recordings=len(minutes), audio_seconds=audio_s, staged_bytes=int(audio_s * 32000))

        def run(leg):
            d = os.path.join(work, "vad_" + leg)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            c0 = time.perf_counter()
            c = ms.make_segments(scp, d, hip_vad=leg)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            return d, time.perf_counter() - c0, c

        if a.only:
            d, el, c = run(a.only)
            print(json.dumps({"only": a.only, "seconds": round(el, 3), "passes": c["passes"], "frames": c["frames"], "staged_bytes": out["staged_bytes"]}))
            return
        legs, dirs = ("device", "host"), {}
        for leg in legs:
            dirs[leg], el, c = run(leg)
            out[leg] = {"first_call_seconds": round(el, 3), "passes": c["passes"], "frames": c["frames"], "segments": c["segments"], "seconds": []}
        for _ in range(max(1, a.runs)):
            for leg in legs:
                out[leg]["seconds"].append(round(run(leg)[1], 4))
        for leg in legs:
            s = out[leg]["seconds"]
            out[leg]["recordings_per_s"] = median_range([round(len(minutes) / x, 2) for x in s])
            out[leg]["audio_s_per_s"] = median_range([round(audio_s / x, 1) for x in s])
        x, y = read_dir(dirs["device"]), read_dir(dirs["host"])
        out["device_and_host_bytes_identical"] = all(x[n] == y[n] for n in ("segments", "vad.ark"))
        assert out["device_and_host_bytes_identical"], "the device leg and the host leg wrote different bytes"
        if a.decode_runs > 0:
            rec = recording(a.decode_minutes, 800)
            long_wav, long_scp, seg_dir = os.path.join(work, "long.wav"), os.path.join(work, "long.scp"), os.path.join(work, "long_vad")
            write_wav(long_wav, rec)
            with open(long_scp, "w") as f:
                f.write("long %s\n" % long_wav)
            ms.make_segments(long_scp, seg_dir, max_segment=10.0)
            seg_file, cut_scp = os.path.join(seg_dir, "segments"), os.path.join(work, "cut.scp")
            os.makedirs(os.path.join(work, "cut"), exist_ok=True)
            segs = segments.read_segments(seg_file)
            with open(cut_scp, "w") as f:
                for utt, _, start, end in segs:
                    first, last = segments.sample_range(start, end, 16000, len(rec), utt, "long")
                    write_wav(os.path.join(work, "cut", utt + ".wav"), rec[first:last])
                    f.write("%s %s\n" % (utt, os.path.join(work, "cut", utt + ".wav")))
            margs = synth.make_args("config2")
            with open(os.path.join(work, "vocab.txt"), "w") as f:
                f.write("".join(f"w{i}\n" for i in range(margs.vocab_size - 4)))
            state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
            torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(work, "model.mdl"))
            keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                    "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
            conf = {k: getattr(margs, k) for k in keys}
            conf.update(vocab_file=os.path.join(work, "vocab.txt"), use_gpu=True)
            cfg = os.path.join(work, "decode.yaml")
            with open(cfg, "w") as f:
                yaml.safe_dump(conf, f)
            forms = {"segments": (long_scp, ["--hip_segments", seg_file]), "cut_files": (cut_scp, [])}
            tasks, out["decode"] = {}, {"segments_of_the_recording": len(segs), "audio_seconds": 60.0 * a.decode_minutes}
            for form, (path, extra) in forms.items():
                cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", path, "--resume_model", os.path.join(work, "model.mdl"),
                       "--batch_size", str(a.decode_batch), "--hip_precision", a.precision, "--hip_max_frames", "1024", "--print_freq", "100000",
                       "--load_data_workers", "0", "--result_file", os.path.join(work, f"result_{form}.txt")] + extra
                args = DecodeParser().get_args(cli)
                for k, v in conf.items():
                    setattr(args, k, v)
                args.test_paths, args.rank = [{"name": "test", "scp_path": path}], 0
                task = CassNATTask("test", args)
                task.load_lm_model(args)
                c0 = time.perf_counter()
                task.decode(args)
                torch.cuda.synchronize()
                tasks[form] = (task, args)
                out["decode"][form] = {"first_call_seconds": round(time.perf_counter() - c0, 3), "seconds": []}
            for _ in range(a.decode_runs):
                for form in forms:
                    task, args = tasks[form]
                    torch.cuda.synchronize()
                    c0 = time.perf_counter()
                    task.decode(args)
                    torch.cuda.synchronize()
                    out["decode"][form]["seconds"].append(round(time.perf_counter() - c0, 4))
            lines = {form: open(tasks[form][1].result_file).read().splitlines() for form in forms}
            out["decode"]["same_lines"] = lines["segments"] == lines["cut_files"]
            for form in forms:
                out["decode"][form].update(median_range(out["decode"][form]["seconds"]))
                tasks[form][0].close()
            out["decode"]["segments_over_cut_files"] = round(out["decode"]["segments"]["median"] / out["decode"]["cut_files"]["median"], 3)
    finally:
        if tmp_ctx is not None:
            tmp_ctx.cleanup()
    out.update(runs=a.runs, note="make_segments in process, reading the files and writing the three output files included; decode: default "
                                 "pipelined decode_asr; profiler off")
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
