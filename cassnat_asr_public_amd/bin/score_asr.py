#!/usr/bin/env python3
"""Score the result file of an earlier run against its references (``utils.score``; what ``decode_asr --hip_score`` does behind a run):

    python -m cassnat_asr_public_amd.bin.score_asr --hyp out/token_results.txt --ref data/test/token.scp \\
        --vocab_file data/dict/vocab.txt --out out/score

writes out/score/wer, per_utt, ref.trn and hyp.trn and prints the %WER line.  ``--host`` aligns with the library's serial host entry
(``cn_edit_align_host``) and needs no GPU; without it the pairs go to the device (``cn_op_edit_align``).  Both write the same files.
"""
import argparse
import sys

from ..data.vocab import Vocab
from ..utils import score
from ..utils.parser import add_score_arguments


def main(argv=None):
    p = argparse.ArgumentParser(description="Score a result file: WER files from the edit alignment")
    p.add_argument("--hyp", required=True, help="the result file of a run: 'UTT piece piece ...' lines")
    p.add_argument("--ref", required=True, help="the reference file: 'UTT unit unit ...' lines")
    p.add_argument("--vocab_file", default="", help="the run's vocabulary (decides whether words can be formed from pieces); without it "
                                                    "--hip_score_unit is taken as given")
    p.add_argument("--out", required=True, help="the directory of the four files")
    p.add_argument("--host", action="store_true", help="align on the host (no GPU)")
    add_score_arguments(p)
    args = p.parse_args(argv)
    vocab = Vocab(args.vocab_file) if args.vocab_file else None
    try:
        score.score_files(args.hyp, args.ref, args.out, vocab, args.hip_score_unit, args.hip_score_ref_form, score.parse_costs(args.hip_score_costs),
                          args.hip_score_mode, args.host)
    except score.ScoreError as e:
        print("score_asr: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
