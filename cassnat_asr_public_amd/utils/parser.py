"""Command-line surface of the recogniser: same flags as the reference's DecodeParser
(src/utils/parser.py:32-54) plus the engine switches of this build."""
import argparse


def add_score_arguments(p):
    """The scorer's options, shared by decode_asr (--hip_score) and bin/score_asr."""
    p.add_argument("--hip_score_unit", default="word", choices=["word", "token", "char"],
                   help="what is counted: word (default; pieces merge at the separator, as in the CTM - a vocabulary without separator "
                        "pieces is scored per token), token (the pieces themselves; needs a reference in pieces) or char (the characters "
                        "of the words)")
    p.add_argument("--hip_score_ref_form", default="pieces", choices=["pieces", "words"],
                   help="the reference file holds pieces (default; what token.scp holds) or words")
    p.add_argument("--hip_score_costs", default="1,1,1", type=str,
                   help="S,I,D: the costs of a substitution, an insertion and a deletion, each in 1 .. 255 (default 1,1,1, Kaldi's "
                        "compute-wer; sclite aligns with 4,3,3).  On equal cost the first of (diagonal, deletion, insertion) wins")
    p.add_argument("--hip_score_mode", default="present", choices=["present", "all"],
                   help="present (default): an utterance of the reference file without a hypothesis is skipped and counted as not "
                        "present; all: its reference counts as deletions")


class DecodeParser(object):
    def __init__(self, description="Decode argument parser"):
        p = argparse.ArgumentParser(description=description)
        p.add_argument("--test_config")
        p.add_argument("--lm_config")
        p.add_argument("--data_path")
        p.add_argument("--text_label", default="", type=str, help="text label")
        p.add_argument("--task", default="cassnat", type=str, help="'cassnat' (NAT) or 'art' (autoregressive transformer): the tasks on the accelerated path")
        p.add_argument("--batch_size", default=32, type=int)
        p.add_argument("--load_data_workers", default=1, type=int)
        p.add_argument("--resume_model", default="", type=str, help="checkpoint with a 'model_state' dict")
        p.add_argument("--result_file", default="", type=str)
        p.add_argument("--print_freq", default=100, type=int)
        p.add_argument("--rnnlm", type=str, default=None)
        p.add_argument("--rank_model", type=str, default="lm")
        p.add_argument("--lm_weight", type=float, default=0.0)
        p.add_argument("--seed", default=1, type=int)
        # engine switches (not in the reference)
        p.add_argument("--hip_precision", default="bf16", choices=["bf16", "fp32", "fp8", "bf16x3", "fp16"],
                       help="fp16: the bf16 engine with half-precision MFMA operands (same speed, operand roundings 8x smaller, range +-65504); bf16 MFMA (throughput), bf16x3 (split-bf16: the reference's tolerance at MFMA speed), fp32 (exact-f32 MFMA), "
                            "fp8 (e4m3 encoder products of the NAT recogniser, BASELINE config 5; a ranking LM / AT model or the "
                            "autoregressive recogniser of --task art run bf16 under it)")
        p.add_argument("--hip_fp8_scope", default="all",
                       help="--hip_precision fp8: which encoder-side products take e4m3 operands - all, or conv2 / linear / "
                            "ffn[:first layer] joined by + (e.g. conv2+ffn:8); fewer products = fewer arg-max flips, less speed-up")
        p.add_argument("--hip_max_frames", default=4096, type=int, help="workspace size in input frames")
        p.add_argument("--hip_pipelines", default=2, type=int,
                       help="decode pipelines per GPU for greedy decoding of a test set (1 = batch after batch, the reference's loop)")
        p.add_argument("--hip_coalesce", default=10, type=int,
                       help="sizes a pipeline's workspace: the area of that many batches of batch_size x 1024 frames; consecutive "
                            "batches - of different frame counts too - share one engine pass while they fit it (every batch's "
                            "hypotheses and scores stay exactly those of a pass of its own)")
        p.add_argument("--hip_ragged", default=0.75, type=float,
                       help="batches share an engine pass while the shortest has at least this fraction of the longest one's frames "
                            "(1 = equal shapes only)")
        p.add_argument("--hip_bucket", default=0, type=int,
                       help="1: form the batches from the utterance list sorted by length (frame counts from <scp dir>/utt2num_frames "
                            "or the ark headers) instead of file order - less padding per batch, neighbours that merge well; the "
                            "result file stays in file order.  0 (default): the reference's batches")
        p.add_argument("--hip_packed_reader", default=1, type=int,
                       help="1 (default): the pipelined decoder reads the utterances' rows straight from the memory-mapped archives into "
                            "page-locked memory, a pass at a time, and pads / normalises on the device - and splices / skips frames there when the "
                            "config asks for it (left_ctx / right_ctx / skip_frame) - for float32 or compressed archives; "
                            "--load_data_workers then sets the number of copy threads; 0: the DataLoader's collated batches")
        p.add_argument("--hip_device_cmvn", default=1, type=int,
                       help="1 (default): the pipelined decoder applies the global CMVN on the device, behind the host-to-device copy "
                            "(float64 arithmetic, bit-identical to the dataset's): on the packed reader, or - for a dataset that neither splices "
                            "nor skips frames - without loader workers; 0: always in the dataset, as the reference does (a spliced set "
                            "then keeps the host path altogether)")
        p.add_argument("--hip_audio", default="auto", choices=["auto", "0", "1"],
                       help="decode from audio: auto (default) - a --data_path whose entries are RIFF/WAVE files (a wav.scp of plain "
                            "paths: 16-bit PCM, one channel) is decoded from the sound files, the Kaldi fbank features computed on the "
                            "device; 0: never look, the entries are feature matrices; 1: the entries must be WAV files")
        p.add_argument("--hip_segments", default="", type=str,
                       help="decode from audio: a Kaldi segments file (`UTT REC START END` lines, seconds, END -1 = the end of the "
                            "recording): the utterances are sample ranges of the WAV recordings --data_path names, cut from the memory "
                            "maps (first = floor(START * rate + 0.5); no file is written); result file, --text_label, --hip_score and "
                            "--hip_bias see segment ids, --hip_ctm writes times in the recording.  A bad segment is an error, not a warning; "
                            "FLAC recordings and a fifth field are refused")
        p.add_argument("--hip_fbank_conf", default="", type=str,
                       help="Kaldi option file of the fbank front-end for audio input (--name=value lines: sample-frequency, frame-length, "
                            "frame-shift, preemphasis-coefficient, remove-dc-offset, window-type, num-mel-bins, low-freq, high-freq, "
                            "use-power, use-log-fbank).  Default: the built-in options, which are those of the reference's conf/fbank.conf "
                            "(hamming window, 16 kHz, 80 mel bins, no energy).  Dither is not implemented: an absent --dither means 0 "
                            "(Kaldi's default of 1.0 adds noise that cannot be compared), a non-zero one is refused")
        p.add_argument("--hip_ctm", default="", type=str,
                       help="also write a CTM file (UTT 1 START DUR WORD CONF): the best hypothesis of every utterance is force-aligned "
                            "to the model's own CTC log-posteriors on the device, word times from the pieces' spans, confidence = exp of "
                            "the smallest piece confidence.  Seconds per subsampled frame = 4 * skip_frame * frame shift (--hip_fbank_conf's, "
                            "else 10 ms); no receptive-field offset.  --task cassnat then keeps the plain loop (like beam search, ESA, LM "
                            "fusion and capture runs: the pipelined greedy path writes no time stamps); the result file does not change")
        p.add_argument("--hip_ctm_unit", default="word", choices=["word", "token"],
                       help="--hip_ctm: word (default; pieces that begin with the separator start a word, a vocabulary without such "
                            "pieces is written per token) or token (one line per piece)")
        p.add_argument("--hip_ctc_merge", default=0, type=int, choices=[0, 1],
                       help="1: the CTC prefix beam search (decode_type ctc_only / ctc_att) merges candidates that spell the same label "
                            "sequence before it ranks them, so the beam holds every sequence once and score_ctc is a prefix probability; "
                            "with and without an n-gram model or --hip_bias.  0 (default): the reference's search, which does not merge")
        p.add_argument("--hip_bias", default="", type=str,
                       help="contextual phrase biasing of the CTC prefix beam search (decode_type ctc_only / ctc_att): a UTF-8 file with "
                            "one phrase per line as vocabulary pieces separated by blanks (e.g. '▁new ▁york'), optionally a tab and a "
                            "per-piece score; empty lines and lines starting with # are skipped.  A hypothesis gains the score per piece "
                            "while it spells a phrase and loses it again when the spelling breaks off")
        p.add_argument("--hip_bias_score", default=3.0, type=float,
                       help="--hip_bias: the per-piece score of a phrase without one of its own (default 3.0; natural-log units, the "
                            "scale of score_ctc)")
        p.add_argument("--hip_bias_search", default="ctc", choices=["ctc", "att"],
                       help="--hip_bias: which search the list biases.  ctc (default): the CTC prefix beam search.  att: the attention "
                            "beam search of --task art, decode_type: ctc_att (the joint CTC / attention search), where a candidate token "
                            "adds what it changes in the open match and eos gives the open match up; every other path refuses att")
        add_score_arguments(p)
        p.add_argument("--hip_score", default="", type=str,
                       help="also score the run against its references: once the result file is written, rank 0 aligns every hypothesis "
                            "with its reference on the device (weighted edit distance) and writes DIR/wer (the lines of Kaldi's compute-wer), "
                            "DIR/per_utt (ref / hyp / op / #csid per utterance), DIR/ref.trn and DIR/hyp.trn; the %%WER line is printed.  A "
                            "post-pass over the result file's strings: every decode path stays available and its files do not change")
        p.add_argument("--hip_score_ref", default="", type=str,
                       help="--hip_score: the reference file, one 'UTT unit unit ...' line per utterance (default: --text_label)")
        p.add_argument("--hip_dist_backend", default="nccl", choices=["nccl", "gloo"],
                       help="torch.distributed backend under torch.distributed.run (nccl = RCCL over xGMI; gloo: rehearsal of the "
                            "N-rank path, also with several ranks on one GPU)")
        self.parser = p

    def get_args(self, argv=None):
        return self.parser.parse_args(argv)
