"""decode_asr from a Kaldi COMPRESSED archive against the float32 archive of the same values: the packed reader's two forms.

    python tools/time_compressed_reader.py [--utts 6000] [--batch 32] [--precision bf16] [--runs 1] [--leg both]

The synthetic test set of tools/ragged_cli_bench.py (ragged utterances of 300..1500 frames, seeded N(0,1) features, the bench's
config-2 model and weights, a global CMVN stats file) is written once as a `CM` archive - what `copy-feats --compress=true` and
steps/make_fbank.sh produce - and once as the `FM ` archive that holds the host-decompressed values.  Both are decoded with the
default pipelined `decode_asr` (in process): the `CM` leg stages one byte per value and decompresses on the device
(cn_op_unpack_compressed), the `FM ` leg stages float32 rows (cn_op_unpack_rows).  The two result files must be identical line for
line.  Prints one JSON line: utt/s per leg (every run and the median), the workers' host seconds by activity (`s_*`) and the
archive bytes.

--runs N alternates the legs N times in one process.  --workdir DIR keeps the archives for further calls; --leg fm with
--package-root TREE runs the float32 leg on another checkout of the package (e.g. the parent commit, which cannot read `CM`): it
only needs the archives this tool has written into --workdir before.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--min-frames", type=int, default=300)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--runs", type=int, default=1, help="timed decodes per leg, the legs alternating")
    ap.add_argument("--leg", default="both", choices=["both", "cm", "fm", "none"], help="none: only write the archives into --workdir")
    ap.add_argument("--workdir", default=None, help="where the archives live (kept; default: a temporary directory)")
    ap.add_argument("--package-root", default=REPO, help="the checkout whose cassnat_asr_public_amd decodes")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    import yaml

    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.data import kaldi_io
    from cassnat_asr_public_amd.tasks import CassNATTask
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    torch.set_num_threads(1)
    margs = synth.make_args("config2")
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(a.min_frames, a.max_frames + 1, size=a.utts)]
    tmp_ctx = tempfile.TemporaryDirectory() if a.workdir is None else None
    work = a.workdir or tmp_ctx.name
    os.makedirs(work, exist_ok=True)
    out = {}
    try:
        scp = {k: os.path.join(work, k + ".scp") for k in ("cm", "fm")}
        done = os.path.join(work, "written_%d" % a.utts)
        t0 = time.perf_counter()
        if not os.path.exists(done):
            def mats():
                for b, n in enumerate(lengths):
                    f, _ = synth.make_feats(1, n, margs.input_size, seed=4000 + b)
                    yield f"spk-utt{b:05d}", f[0]

            kaldi_io.write_ark_scp(os.path.join(work, "cm.ark"), scp["cm"], mats(), compress=1)
            kaldi_io.write_ark_scp(os.path.join(work, "fm.ark"), scp["fm"], ((u, kaldi_io.load_mat(s)) for u, s in kaldi_io.read_scp(scp["cm"])))
            n = float(sum(lengths))  # Kaldi global CMVN stats (sums, sums of squares, count) of N(0.2, 1.5^2) features
            stats = np.zeros((2, margs.input_size + 1))
            stats[0, :-1], stats[0, -1], stats[1, :-1] = 0.2 * n, n, (1.5 ** 2 + 0.2 ** 2) * n
            kaldi_io.write_ark_scp(os.path.join(work, "cmvn.ark"), os.path.join(work, "cmvn.scp"), [("global", stats)])
            with open(os.path.join(work, "vocab.txt"), "w") as f:
                f.write("".join(f"w{i}\n" for i in range(margs.vocab_size - 4)))
            state = synth.make_state(margs, seed=0, blank_bias=synth.BENCH_BLANK_BIAS)
            torch.save({"model_state": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(work, "model.mdl"))
            open(done, "w").close()
        out["setup_s"] = round(time.perf_counter() - t0, 1)
        out["archive_bytes"] = {k: os.path.getsize(os.path.join(work, k + ".ark")) for k in ("cm", "fm")}
        keys = ("input_size", "d_model", "n_head", "d_ff", "N_enc", "model_type", "n_features", "left_ctx", "right_ctx", "skip_frame",
                "padding_idx", "beam_width", "length_penalty", "d_encff", "d_decff", "N_extra", "N_self_dec", "N_mix_dec", "use_trigger")
        conf = {k: getattr(margs, k) for k in keys}
        conf.update(vocab_file=os.path.join(work, "vocab.txt"), use_gpu=True, use_cmvn=True,
                    global_cmvn=kaldi_io.read_scp(os.path.join(work, "cmvn.scp"))[0][1])
        cfg = os.path.join(work, "decode.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump(conf, f)
        legs = {"both": ["fm", "cm"], "cm": ["cm"], "fm": ["fm"], "none": []}[a.leg]
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
            task = CassNATTask("test", args)
            task.load_lm_model(args)
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            task.decode(args)  # the first call creates engines, workspaces, threads and the row-count predictor
            torch.cuda.synchronize()
            tasks[leg] = (task, args)
            out[leg] = {"first_call_seconds": round(time.perf_counter() - c0, 3), "seconds": [], "utt_per_s": [], "worker_host_seconds": []}
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
                rec["engine_passes"], rec["compressed_passes"] = st["passes"], st.get("compressed_passes", 0)
        for leg in legs:
            task, args = tasks[leg]
            results[leg] = open(args.result_file).read().splitlines()
            assert len(results[leg]) == a.utts
            out[leg]["utt_per_s_median"] = statistics.median(out[leg]["utt_per_s"])
            task.close()
        if "cm" in legs:
            assert out["cm"]["compressed_passes"] == out["cm"]["engine_passes"] > 0, "the CM leg did not take the compressed packed reader"
        for leg in ("cm", "fm"):  # (a leg run by an earlier call on the same --workdir left its result file there)
            path = os.path.join(work, f"result_{leg}.txt")
            if leg not in results and legs and os.path.exists(path):
                results[leg] = open(path).read().splitlines()
        if len(results) == 2:
            assert results["cm"] == results["fm"], "result files differ between the CM archive and the FM archive of its values"
            out["result_files_identical"] = True
    finally:
        if tmp_ctx is not None:
            tmp_ctx.cleanup()
    out.update(utterances=a.utts, batch_size=a.batch, precision=a.precision, frames_min_max=[min(lengths), max(lengths)], legs=legs,
               package_root=os.path.relpath(os.path.abspath(a.package_root), REPO),
               note="default pipelined decode_asr, reading the ark included; fm = the float32 archive of the CM archive's decompressed values")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
