"""decode_asr from a `wav.scp` against the float32 archive of the same features: the packed reader's wave form beside its float32 form.

    python tools/time_wave_reader.py [--utts 6000] [--batch 32] [--precision bf16] [--runs 6] [--leg both] [--out FILE.jsonl]

The ragged test set of tools/time_compressed_reader.py (utterances of 300..1500 frames, same seed and lengths, the bench's config-2
model and weights, a global CMVN stats file) is written twice: as one 16-bit RIFF/WAVE file per utterance (seeded noise on top of a
few sines, exactly the samples that give the utterance's frame count) and as the `FM ` archive of the features the device computes
from those files (`Fbank.packed`, no CMVN).  Both are decoded with the default pipelined `decode_asr` (in process): the wave leg
stages the int16 samples and runs cn_op_fbank_packed, the `FM ` leg stages float32 rows (cn_op_unpack_rows) - the same number of
bytes at the default options.  The two result files must be identical line for line.  Prints one JSON line (and appends it to
--out): utt/s per leg (every run, median, range) and the workers' host seconds by activity.

--runs N alternates the legs N times in one process.  --workdir DIR keeps the files for further calls.
"""
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
    head = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", len(data))
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(head) + len(data)) + head + data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--min-frames", type=int, default=300)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--runs", type=int, default=6, help="timed decodes per leg, the legs alternating")
    ap.add_argument("--leg", default="both", choices=["both", "wav", "fm", "none"], help="none: only write the files into --workdir")
    ap.add_argument("--workdir", default=None, help="where the files live (kept; default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    import yaml

    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.data import kaldi_io, wave_io
    from cassnat_asr_public_amd.data.fbank import Fbank
    from cassnat_asr_public_amd.tasks import CassNATTask
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    torch.set_num_threads(1)
    margs = synth.make_args("config2")
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(a.min_frames, a.max_frames + 1, size=a.utts)]
    tmp_ctx = tempfile.TemporaryDirectory() if a.workdir is None else None
    work = a.workdir or tmp_ctx.name
    os.makedirs(os.path.join(work, "wav"), exist_ok=True)
    out = {}
    try:
        scp = {k: os.path.join(work, k + ".scp") for k in ("wav", "fm")}
        done = os.path.join(work, "written_%d" % a.utts)
        t0 = time.perf_counter()
        if not os.path.exists(done):
            t = np.arange(400 + 160 * (a.max_frames - 1)) / 16000.0
            with open(scp["wav"], "w") as f:
                for b, n in enumerate(lengths):
                    g = np.random.default_rng(4000 + b)
                    ns = 400 + 160 * (n - 1)
                    w = 600.0 * g.standard_normal(ns)
                    for amp, freq in zip(g.uniform(300, 3000, 3), g.uniform(80, 7000, 3)):
                        w += amp * np.sin(2 * np.pi * freq * t[:ns])
                    path = os.path.join(work, "wav", f"spk-utt{b:05d}.wav")
                    write_wav(path, np.clip(np.rint(w), -32768, 32767))
                    f.write(f"spk-utt{b:05d} {path}\n")
            fb = Fbank()
            entries = kaldi_io.read_scp(scp["wav"])
            sums, sq, count = np.zeros(80), np.zeros(80), 0.0

            def mats():
                nonlocal sums, sq, count
                for i in range(0, len(entries), 64):
                    chunk = entries[i:i + 64]
                    views = [wave_io.pcm_view(p, 16000, u) for u, p in chunk]
                    feats, _ = fb.packed(views)
                    feats = feats.cpu().numpy()
                    for (u, _), v, m in zip(chunk, views, feats):
                        m = m[: fb.num_frames(len(v))]
                        m64 = m.astype(np.float64)
                        sums, sq, count = sums + m64.sum(0), sq + (m64 ** 2).sum(0), count + len(m)
                        yield u, m

            kaldi_io.write_ark_scp(os.path.join(work, "fm.ark"), scp["fm"], mats())
            stats = np.zeros((2, 81))  # Kaldi global CMVN stats (sums, sums of squares, count) of the device's features
            stats[0, :-1], stats[0, -1], stats[1, :-1] = sums, count, sq
            kaldi_io.write_ark_scp(os.path.join(work, "cmvn.ark"), os.path.join(work, "cmvn.scp"), [("global", stats)])
            with open(os.path.join(work, "vocab.txt"), "w") as f:
                f.write("".join(f"w{i}\n" for i in range(margs.vocab_size - 4)))
            state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
            torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(work, "model.mdl"))
            open(done, "w").close()
        out["setup_s"] = round(time.perf_counter() - t0, 1)
        out["bytes"] = {"wav": sum(os.path.getsize(p) for _, p in kaldi_io.read_scp(scp["wav"])), "fm": os.path.getsize(os.path.join(work, "fm.ark"))}
        keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
        conf = {k: getattr(margs, k) for k in keys}
        conf.update(vocab_file=os.path.join(work, "vocab.txt"), use_gpu=True, use_cmvn=True,
                    global_cmvn=kaldi_io.read_scp(os.path.join(work, "cmvn.scp"))[0][1])
        cfg = os.path.join(work, "decode.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump(conf, f)
        legs = {"both": ["fm", "wav"], "wav": ["wav"], "fm": ["fm"], "none": []}[a.leg]
        tasks, results = {}, {}
        for leg in legs:
            cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp[leg], "--resume_model", os.path.join(work, "model.mdl"),
                   "--batch_size", str(a.batch), "--hip_precision", a.precision, "--hip_bucket", "1", "--hip_max_frames", str(a.max_frames),
                   "--print_freq", "100000", "--load_data_workers", "0", "--result_file", os.path.join(work, f"result_{leg}.txt")]
            args = DecodeParser().get_args(cli)
            for k, v in conf.items():
                setattr(args, k, v)
            args.test_paths = [{"name": "test", "scp_path": scp[leg]}]
            args.rank = 0
            c0 = time.perf_counter()
            task = CassNATTask("test", args)
            task.load_lm_model(args)
            torch.cuda.synchronize()
            c1 = time.perf_counter()
            task.decode(args)  # the first call creates engines, workspaces, threads and the row-count predictor
            torch.cuda.synchronize()
            tasks[leg] = (task, args)
            out[leg] = {"task_seconds": round(c1 - c0, 3), "first_call_seconds": round(time.perf_counter() - c1, 3), "seconds": [],
                        "utt_per_s": [], "worker_host_seconds": []}
        for _ in range(max(1, a.runs)):
            for leg in legs:
                task, args = tasks[leg]
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                task.decode(args)
                torch.cuda.synchronize()
                el = time.perf_counter() - c0
                rec, st = out[leg], task.pipeline_stats
                rec["seconds"].append(round(el, 4))
                rec["utt_per_s"].append(round(a.utts / el, 1))
                rec["worker_host_seconds"].append({k: round(v, 3) for k, v in st.items() if k.startswith("s_")})
                rec["engine_passes"], rec["wave_passes"] = st["passes"], st.get("wave_passes", 0)
        for leg in legs:
            task, args = tasks[leg]
            results[leg] = open(args.result_file).read().splitlines()
            assert len(results[leg]) == a.utts
            out[leg]["utt_per_s_median"] = statistics.median(out[leg]["utt_per_s"])
            out[leg]["utt_per_s_range"] = [min(out[leg]["utt_per_s"]), max(out[leg]["utt_per_s"])]
            task.close()
        if "wav" in legs:
            assert out["wav"]["wave_passes"] == out["wav"]["engine_passes"] > 0, "the wave leg did not take the packed reader's wave form"
        if len(results) == 2:
            assert results["wav"] == results["fm"], "result files differ between the wav.scp and the FM archive of its features"
            out["result_files_identical"] = True
    finally:
        if tmp_ctx is not None:
            tmp_ctx.cleanup()
    out.update(utterances=a.utts, batch_size=a.batch, precision=a.precision, frames_min_max=[min(lengths), max(lengths)], legs=legs,
               runs=a.runs, note="default pipelined decode_asr, reading the files included; fm = the float32 archive of the device's own "
                                 "fbank features of the WAV files; profiler off")
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
