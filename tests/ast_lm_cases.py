"""The seeded inputs of the LM-fusion fixtures of the AST beam search (tools/make_ast_lm_goldens.py writes them from the
reference; tests/test_gpu_ast_lm.py reads them).  Every case returns (args, state, feats, lm_args, lm_state, precision-free
description); lm_args is None for the no-LM widening case."""
import numpy as np

from cassnat_asr_public_amd import synth


def _tiny(**ov):
    args = synth.make_args_ast("tiny_ast", beam_width=3, ctc_beam=5, max_decode_ratio=0.75, **ov)
    state = synth.make_state(args, seed=3, gain=2.0)
    feats, _ = synth.make_feats(3, 61, 80, lengths=[61, 57, 51], seed=11)
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=args.vocab_size)
    lm_state = synth.make_state(lm_args, seed=9, gain=2.0)
    return args, state, feats, lm_args, lm_state, "tiny_ast + tiny_lm"


def _c4(lm, **ov):
    args = synth.make_args_ast("config4", max_decode_ratio=0.3, **ov)
    state = synth.make_state(args, seed=5)
    feats, _ = synth.make_feats(2, 400, 80, lengths=[400, 333], seed=31)
    if lm is None:
        return args, state, feats, None, None, "config4, no LM"
    lm_args = synth.make_args_lm(lm, vocab_size=args.vocab_size)
    return args, state, feats, lm_args, synth.make_state(lm_args, seed=9), "config4 + " + lm


def _conf_recipe():
    # run_art.sh stage 3's shape family: config-4 decoder behind a conformer encoder (N_enc 3, as conf_ast_c4), the lm.yaml LM
    # with 4 of its 16 layers, conf/decode.yaml's beam 20 / ctc_beam 30, ctc_weight 0.4, lm_weight 0.6
    args = synth.make_args_ast("config4_conf", N_enc=3, max_decode_ratio=0.3, ctc_weight=0.4, lm_weight=0.6, beam_width=20,
                               ctc_beam=30)
    state = synth.make_state(args, seed=5)
    feats, _ = synth.make_feats(4, 300, 80, lengths=[300, 287, 262, 231], seed=31)
    lm_args = synth.make_args_lm("lm_recipe", N=4, vocab_size=args.vocab_size)
    return args, state, feats, lm_args, synth.make_state(lm_args, seed=9), "config4_conf + lm_recipe (N 4)"


CASES = {
    "ast_lm_tiny_att": lambda: _tiny(ctc_weight=0.0, lm_weight=0.6),
    "ast_lm_tiny_ctc": lambda: _tiny(ctc_weight=0.4, lm_weight=0.6),
    "ast_lm_tiny_lp": lambda: _tiny(ctc_weight=0.5, length_penalty=0.2, T=1.3, lm_weight=0.3),
    "ast_lm_c4": lambda: _c4("lm_small", ctc_weight=0.3, lm_weight=0.5, beam_width=10),
    "ast_wide_c4": lambda: _c4(None, ctc_weight=0.3, beam_width=20, ctc_beam=30),
    "conf_ast_lm_recipe": _conf_recipe,
}


def lm_step_prefixes():
    """Token rows of ast_lm_step_tiny: sos first, tokens of the tiny vocabulary (40), some blanks (0) inside the prefix."""
    rng = np.random.default_rng(21)
    ys = rng.integers(3, 40, size=(6, 9)).astype(np.int32)
    ys[:, 0] = 1
    ys[1, 3] = 0
    ys[2, 1] = 0
    ys[2, 5] = 0
    ys[4, 8] = 0
    return ys
