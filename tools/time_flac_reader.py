"""decode_asr from a `wav.scp` of FLAC files against the WAV files of the same samples: the packed reader's FLAC form beside its wave form.

    python tools/time_flac_reader.py [--utts 6000] [--batch 32] [--precision bf16] [--runs 5] [--leg both] [--out FILE.jsonl]

The ragged test set of the other reader tools (utterances of 300..1500 frames, same seed and lengths, the bench's config-2 model and
weights, a global CMVN stats file) is written twice: as one 16-bit RIFF/WAVE file per utterance and as one FLAC file per utterance
holding the same samples, written by the vectorised writer of the tests' model of the format (tests/flac_model.py: fixed predictor of
order 2, one Rice partition per block of 4096; entries alternate between plain paths and the recipe's `flac -c -d -s FILE |`).  The
signal is speech-like - noise through an autoregressive filter, amplitude-modulated, with pauses - so that the streams compress about
as LibriSpeech does; the tool prints the ratio it got (white noise would not compress and would measure nothing).  Both sets are
decoded with the default pipelined `decode_asr` (in process; bf16, --hip_coalesce 4, --hip_bucket 1): the FLAC leg stages the files'
frames and their table and runs cn_op_flac_decode in front of cn_op_fbank_packed, the WAV leg stages the int16 samples.  The two
result files must be identical line for line.  Prints one JSON line (and appends it to --out): utt/s per leg (every run, median,
range), staged bytes per utterance, the workers' host seconds by activity.

--runs N alternates the legs N times in one process.  --workdir DIR keeps the files for further calls (encoded once, reused).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def speech_like(n, seed):
    """n int16 samples: white noise through a decaying (autoregressive-like) filter, a slow amplitude envelope, silent pauses."""
    g = np.random.default_rng(seed)
    taps = 0.95 ** np.arange(96)  # (twice through a pole at 0.95: the order-2 predictor then leaves about half the bits, as on speech)
    x = np.convolve(np.convolve(g.standard_normal(n + 95), taps, mode="valid"), taps, mode="same") * 75.0
    t = np.arange(n) / 16000.0
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * g.uniform(1.5, 4.0) * t + g.uniform(0, 6.28))
    for start in g.integers(0, max(1, n - 4000), size=max(1, n // 40000)):
        x[start:start + int(g.integers(1500, 4000))] *= 0.01  # a pause
    return np.clip(np.rint(x), -32768, 32767).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--min-frames", type=int, default=300)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--runs", type=int, default=5, help="timed decodes per leg, the legs alternating")
    ap.add_argument("--leg", default="both", choices=["both", "flac", "wav", "none"], help="none: only write the files into --workdir")
    ap.add_argument("--workdir", default=None, help="where the files live (kept; default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import yaml

    import flac_model
    from time_wave_reader import write_wav
    from cassnat_asr_public_amd import hip, synth
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
    for d in ("wav", "flac"):
        os.makedirs(os.path.join(work, d), exist_ok=True)
    out = {}
    try:
        scp = {k: os.path.join(work, k + ".scp") for k in ("wav", "flac")}
        done = os.path.join(work, "written_%d" % a.utts)
        t0 = time.perf_counter()
        if not os.path.exists(done):
            with open(scp["wav"], "w") as fw, open(scp["flac"], "w") as ff:
                for b, n in enumerate(lengths):
                    x = speech_like(400 + 160 * (n - 1), 4000 + b)
                    wpath, fpath = os.path.join(work, "wav", f"spk-utt{b:05d}.wav"), os.path.join(work, "flac", f"spk-utt{b:05d}.flac")
                    write_wav(wpath, x)
                    with open(fpath, "wb") as f:
                        f.write(flac_model.encode_fast(x, crc16_fn=hip.flac_crc16)[0])
                    fw.write(f"spk-utt{b:05d} {wpath}\n")
                    ff.write(f"spk-utt{b:05d} {fpath}\n" if b % 2 else f"spk-utt{b:05d} flac -c -d -s {fpath} |\n")
            fb = Fbank()
            entries = kaldi_io.read_scp(scp["wav"])
            sums, sq, count = np.zeros(80), np.zeros(80), 0.0
            for i in range(0, len(entries), 64):  # the global CMVN statistics of the device's own features
                views = [wave_io.pcm_view(p, 16000, u) for u, p in entries[i:i + 64]]
                feats = fb.packed(views)[0].cpu().numpy()
                for v, m in zip(views, feats):
                    m64 = m[: fb.num_frames(len(v))].astype(np.float64)
                    sums, sq, count = sums + m64.sum(0), sq + (m64 ** 2).sum(0), count + len(m64)
            stats = np.zeros((2, 81))
            stats[0, :-1], stats[0, -1], stats[1, :-1] = sums, count, sq
            kaldi_io.write_ark_scp(os.path.join(work, "cmvn.ark"), os.path.join(work, "cmvn.scp"), [("global", stats)])
            with open(os.path.join(work, "vocab.txt"), "w") as f:
                f.write("".join(f"w{i}\n" for i in range(margs.vocab_size - 4)))
            state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
            torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(work, "model.mdl"))
            open(done, "w").close()
        out["setup_s"] = round(time.perf_counter() - t0, 1)
        size = {k: sum(os.path.getsize(os.path.join(work, k, n)) for n in os.listdir(os.path.join(work, k))) for k in ("wav", "flac")}
        out["file_bytes_per_utt"] = {k: round(v / a.utts) for k, v in size.items()}
        out["compression_ratio"] = round(size["flac"] / size["wav"], 3)
        keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
        conf = {k: getattr(margs, k) for k in keys}
        conf.update(vocab_file=os.path.join(work, "vocab.txt"), use_gpu=True, use_cmvn=True,
                    global_cmvn=kaldi_io.read_scp(os.path.join(work, "cmvn.scp"))[0][1])
        cfg = os.path.join(work, "decode.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump(conf, f)
        legs = {"both": ["flac", "wav"], "flac": ["flac"], "wav": ["wav"], "none": []}[a.leg]
        tasks, results = {}, {}
        for leg in legs:
            cli = ["--task", "cassnat", "--test_config", cfg, "--data_path", scp[leg], "--resume_model", os.path.join(work, "model.mdl"),
                   "--batch_size", str(a.batch), "--hip_precision", a.precision, "--hip_bucket", "1", "--hip_coalesce", "4",
                   "--hip_max_frames", str(a.max_frames), "--print_freq", "100000", "--load_data_workers", "0",
                   "--result_file", os.path.join(work, f"result_{leg}.txt")]
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
                rec["engine_passes"], rec["wave_passes"], rec["flac_passes"] = st["passes"], st.get("wave_passes", 0), st.get("flac_passes", 0)
        for leg in legs:
            task, args = tasks[leg]
            results[leg] = open(args.result_file).read().splitlines()
            assert len(results[leg]) == a.utts
            out[leg]["utt_per_s_median"] = statistics.median(out[leg]["utt_per_s"])
            out[leg]["utt_per_s_range"] = [min(out[leg]["utt_per_s"]), max(out[leg]["utt_per_s"])]
            # what crosses to the device per utterance: the files' frames (and 16 bytes of table per frame), or the int16 samples
            table = 16 * sum(-(-(400 + 160 * (n - 1)) // 4096) for n in lengths) / a.utts  # (16 bytes of frame table per block of 4096 samples)
            out[leg]["staged_bytes_per_utt"] = round(out["file_bytes_per_utt"][leg] + (table - 42 if leg == "flac" else -44))
            task.close()
        if "flac" in legs:
            assert out["flac"]["flac_passes"] == out["flac"]["engine_passes"] > 0, "the FLAC leg did not take the packed reader's FLAC form"
        if len(results) == 2:
            assert results["flac"] == results["wav"], "result files differ between the FLAC files and the WAV files of the same samples"
            out["result_files_identical"] = True
    finally:
        if tmp_ctx is not None:
            tmp_ctx.cleanup()
    out.update(utterances=a.utts, batch_size=a.batch, precision=a.precision, frames_min_max=[min(lengths), max(lengths)], legs=legs,
               runs=a.runs, note="default pipelined decode_asr, reading and indexing the files included; flac = the same samples as the WAV "
                                 "files, written by tests/flac_model.py encode_fast; profiler off")
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
