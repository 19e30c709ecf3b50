"""bin/make_fbank on the ragged test set of the reader tools, and decode_asr from the archive it writes beside decode_asr from the audio.

    python tools/time_make_fbank.py [--utts 6000] [--batch 64] [--runs 5] [--sources wav,flac] [--legs device,host,false]
                                    [--decode-runs 5] [--out profiles/make_fbank_time.jsonl] [--workdir DIR]

The set is the one of tools/time_wave_reader.py / tools/time_flac_reader.py (utterances of 300..1500 frames, same seed, lengths and
speech-like signal), written once as 16-bit WAV files and as FLAC files of the same samples.  Legs, taking turns in one process,
--runs times each per source:
    device   --hip_compress device: compression and statistics by the kernels, one copy of payloads and sums back
    host     --hip_compress host: the float32 rows come back and the serial twins run (the baseline: the parent commit has no tool)
    false    --compress false: float32 `FM ` rows
Every run writes the whole directory (feats.ark, feats.scp, utt2num_frames, cmvn.ark); the device and the host leg must write the
same bytes.  Then the `CM` archive of the FLAC source and the FLAC wav.scp itself are decoded with the same model (the bench's
config-2 weights, bf16, the archive's own cmvn.ark), alternating --decode-runs times: "features once, decode many" on this tree.
Prints one JSON line (and appends it to --out): utt/s per leg (every run, median, range), the bytes copied back per utterance.

--only LEG --source SRC: that one leg once, nothing else - the run to put under `rocprofv3 --kernel-trace --stats` (on its own: a
profiler changes the timings of everything else)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_set(work, lengths):
    import flac_model
    from time_flac_reader import speech_like
    from time_wave_reader import write_wav
    from cassnat_asr_public_amd import hip

    scp = {k: os.path.join(work, k + ".scp") for k in ("wav", "flac")}
    done = os.path.join(work, "written_%d" % len(lengths))
    if not os.path.exists(done):
        for d in ("wav", "flac"):
            os.makedirs(os.path.join(work, d), exist_ok=True)
        with open(scp["wav"], "w") as fw, open(scp["flac"], "w") as ff:
            for b, n in enumerate(lengths):
                x = speech_like(400 + 160 * (n - 1), 4000 + b)
                wpath, fpath = os.path.join(work, "wav", f"spk-utt{b:05d}.wav"), os.path.join(work, "flac", f"spk-utt{b:05d}.flac")
                write_wav(wpath, x)
                with open(fpath, "wb") as f:
                    f.write(flac_model.encode_fast(x, crc16_fn=hip.flac_crc16)[0])
                fw.write(f"spk-utt{b:05d} {wpath}\n")
                ff.write(f"spk-utt{b:05d} {fpath}\n" if b % 2 else f"spk-utt{b:05d} flac -c -d -s {fpath} |\n")
        open(done, "w").close()
    return scp


def summary(rec):
    rec["utt_per_s_median"] = statistics.median(rec["utt_per_s"])
    rec["utt_per_s_range"] = [min(rec["utt_per_s"]), max(rec["utt_per_s"])]


def read_dir(path):
    return {n: open(os.path.join(path, n), "rb").read() for n in sorted(os.listdir(path))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--min-frames", type=int, default=300)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sources", default="wav,flac")
    ap.add_argument("--legs", default="device,host,false")
    ap.add_argument("--decode-runs", type=int, default=5, help="0: no decode comparison")
    ap.add_argument("--decode-batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--only", default=None, choices=["device", "host", "false"], help="run that leg once on --source and stop (for a profiler)")
    ap.add_argument("--source", default="wav", choices=["wav", "flac"])
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import torch
    import yaml

    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.bin import make_fbank as mf
    from cassnat_asr_public_amd.tasks import CassNATTask
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    torch.set_num_threads(1)
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(a.min_frames, a.max_frames + 1, size=a.utts)]
    tmp_ctx = tempfile.TemporaryDirectory() if a.workdir is None else None
    work = a.workdir or tmp_ctx.name
    os.makedirs(work, exist_ok=True)
    out = {}
    try:
        t0 = time.perf_counter()
        scp = write_set(work, lengths)
        out["setup_s"] = round(time.perf_counter() - t0, 1)

        def run(src, leg, tag=""):
            d = os.path.join(work, "fbank_%s_%s%s" % (src, leg, tag))
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            c = mf.make_fbank(scp[src], d, compress=leg != "false", batch_size=a.batch, hip_compress="host" if leg == "host" else "device")
            torch.cuda.synchronize()
            return d, time.perf_counter() - c0, c

        if a.only:
            d, el, c = run(a.source, a.only, "_once")
            print(json.dumps({"only": a.only, "source": a.source, "seconds": round(el, 3), "passes": c["passes"], "utterances": a.utts}))
            return
        sources, legs = a.sources.split(","), a.legs.split(",")
        dirs = {}
        for src in sources:
            out[src] = {leg: {"seconds": [], "utt_per_s": []} for leg in legs}
            for leg in legs:  # (a first call each: buffers, page-locked memory, the files into the page cache)
                dirs[(src, leg)], el, c = run(src, leg)
                out[src][leg].update(first_call_seconds=round(el, 3), passes=c["passes"], bytes_back_per_utt=round(c["bytes_back"] / a.utts),
                                     archive_bytes_per_utt=round(os.path.getsize(os.path.join(dirs[(src, leg)], "feats.ark")) / a.utts))
            for _ in range(max(1, a.runs)):
                for leg in legs:
                    _, el, _ = run(src, leg)
                    out[src][leg]["seconds"].append(round(el, 4))
                    out[src][leg]["utt_per_s"].append(round(a.utts / el, 1))
            for leg in legs:
                summary(out[src][leg])
            if "device" in legs and "host" in legs:
                x, y = read_dir(dirs[(src, "device")]), read_dir(dirs[(src, "host")])
                # (the scp names its own directory: compare the archives, the frame table and the statistics)
                out[src]["device_and_host_bytes_identical"] = all(x[n] == y[n] for n in ("feats.ark", "utt2num_frames", "cmvn.ark"))
                assert out[src]["device_and_host_bytes_identical"], "the device leg and the host leg wrote different bytes"
        if a.decode_runs > 0 and ("flac", "device") in dirs:
            margs = synth.make_args("config2")
            with open(os.path.join(work, "vocab.txt"), "w") as f:
                f.write("".join(f"w{i}\n" for i in range(margs.vocab_size - 4)))
            state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
            torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(work, "model.mdl"))
            keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                    "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
            conf = {k: getattr(margs, k) for k in keys}
            arch = dirs[("flac", "device")]
            conf.update(vocab_file=os.path.join(work, "vocab.txt"), use_gpu=True, use_cmvn=True, global_cmvn=os.path.join(arch, "cmvn.ark"))
            cfg = os.path.join(work, "decode.yaml")
            with open(cfg, "w") as f:
                yaml.safe_dump(conf, f)
            paths = {"cm_archive": os.path.join(arch, "feats.scp"), "flac_audio": scp["flac"]}
            tasks = {}
            out["decode"] = {}
            for leg, path in paths.items():
                cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", path, "--resume_model", os.path.join(work, "model.mdl"),
                       "--batch_size", str(a.decode_batch), "--hip_precision", a.precision, "--hip_bucket", "1", "--hip_coalesce", "4",
                       "--hip_max_frames", str(a.max_frames), "--print_freq", "100000", "--load_data_workers", "0",
                       "--result_file", os.path.join(work, f"result_{leg}.txt")]
                args = DecodeParser().get_args(cli)
                for k, v in conf.items():
                    setattr(args, k, v)
                args.test_paths = [{"name": "test", "scp_path": path}]
                args.rank = 0
                task = CassNATTask("test", args)
                task.load_lm_model(args)
                c0 = time.perf_counter()
                task.decode(args)
                torch.cuda.synchronize()
                tasks[leg] = (task, args)
                out["decode"][leg] = {"first_call_seconds": round(time.perf_counter() - c0, 3), "seconds": [], "utt_per_s": []}
            for _ in range(a.decode_runs):
                for leg in paths:
                    task, args = tasks[leg]
                    torch.cuda.synchronize()
                    c0 = time.perf_counter()
                    task.decode(args)
                    torch.cuda.synchronize()
                    el = time.perf_counter() - c0
                    out["decode"][leg]["seconds"].append(round(el, 4))
                    out["decode"][leg]["utt_per_s"].append(round(a.utts / el, 1))
            for leg in paths:
                summary(out["decode"][leg])
                assert len(open(tasks[leg][1].result_file).read().splitlines()) == a.utts
                tasks[leg][0].close()
    finally:
        if tmp_ctx is not None:
            tmp_ctx.cleanup()
    out.update(utterances=a.utts, batch_size=a.batch, frames_min_max=[min(lengths), max(lengths)], runs=a.runs,
               note="make_fbank in process, reading (and for FLAC indexing) the files and writing the four output files included; "
                    "decode: default pipelined decode_asr, bf16; profiler off")
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
