"""Inputs of the packed-decoder-rows tests (test_gpu_packed_decoder.py): the config-2 architecture (the row chain needs d_model
256) on eight utterances of 40 to 400 frames, chosen on the CPU with the oracle so that the row counts cover what the packed
layout has to get right - see ``check_row_counts``."""
import numpy as np

from cassnat_asr_public_amd import synth

BLANK_BIAS = 0.35
LENGTHS = [400, 390, 300, 200, 120, 60, 40, 40]
FEAT_SEED = 9000
SILENT = 7  # this utterance's features are scaled to ~0: the blank bias decides every frame, no token, ylen = 1 (the EOS row)
# the merged pass: the first four utterances as one batch of 400 frames, four others as a batch of 312 frames
MERGED_LENGTHS = [312, 250, 97, 40]
MERGED_SEED = 9100


def subsampled(T):
    return ((T - 1) // 2 + 1 - 1) // 2 + 1


def make_case():
    args = synth.make_args("config2")
    args.hip_max_batch, args.hip_max_frames = 8, 400
    state = synth.make_state(args, seed=0, blank_bias=BLANK_BIAS)
    feats, sizes = synth.make_feats(len(LENGTHS), LENGTHS[0], 80, lengths=LENGTHS, seed=FEAT_SEED)
    feats[SILENT] *= 1e-3
    return args, state, feats, sizes


def make_merged_case():
    """(feats (8, 400, 80), sizes, rows, frames, the two batches as they would be decoded alone)."""
    _, _, feats, sizes = make_case()
    a = (feats[:4].copy(), sizes[:4].copy())
    fb, sb = synth.make_feats(len(MERGED_LENGTHS), MERGED_LENGTHS[0], 80, lengths=MERGED_LENGTHS, seed=MERGED_SEED)
    merged = np.zeros((8, 400, 80), np.float32)
    merged[:4] = a[0]
    merged[4:, : fb.shape[1]] = fb
    return merged, np.concatenate([a[1], sb]), [4, 4], [400, fb.shape[1]], [a, (fb, sb)]


def rows_read(ylen, limit=None):
    """r[b] = min(ylen[b] + 1, largest ylen of the batch): the rows the greedy finish reads of every utterance."""
    ylen = np.asarray(ylen, np.int64)
    lim = int(ylen.max()) if limit is None else int(limit)
    return np.minimum(ylen + 1, lim)


def check_row_counts(ylen):
    """Conditions on the INPUTS (the oracle's row counts), not on the code under test."""
    ylen = np.asarray(ylen, np.int64)
    assert (ylen <= 2).any(), ylen                    # an utterance of one or two rows
    assert ((ylen > 32) & (ylen <= 64)).any(), ylen   # one whose keys end inside the first 64-key tile
    assert (ylen > 64).any(), ylen                    # one with a second key tile
    total = int(rows_read(ylen).sum())
    assert total > 128 and total % 32 != 0, total     # more than one row-kernel workgroup, a ragged last 32-row block
    return total
