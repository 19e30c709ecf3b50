"""The seeded inputs of the CTC prefix beam search + LM fixtures (tools/make_ctc_lm_goldens.py writes them from the reference's
own ctc_beam_decode with a TransformerLM as lm_model; tests/test_ctc_lm_model.py and tests/test_gpu_ctc_lm.py read them).  Every
case returns (args, state, feats, sizes, lm_args, lm_state, extra), as tests/nat_lm_cases.py does.

The tiny cases are chosen so that no two neighbouring sort keys among the first ctc_beam + 1 candidates of any frame lie closer
than 1e-3 (the generator refuses to write the fixture otherwise): every beam entry is then the reference's on the fp32 and
split-bf16 engines, whose log-posteriors are within 1e-5."""
from cassnat_asr_public_amd import synth

TINY_BATCH = (3, 61, [61, 50, 37])


def _tiny(preset="tiny", seed=2, blank_bias=None, extra=None, **ov):
    ov.setdefault("decode_type", "ctc_only")
    ov.setdefault("ctc_lm_weight", 0.3)
    ov.setdefault("ctc_beam", 5)
    ov.setdefault("ctc_pruning", 8)
    ov.setdefault("ctc_lp", 0.2)
    ov.setdefault("lm_weight", 0)
    args = synth.make_args(preset, **ov)
    kw = {} if blank_bias is None else dict(blank_bias=blank_bias)
    state = synth.make_state(args, seed=seed, gain=2.0, **kw)
    feats, sizes = synth.make_feats(TINY_BATCH[0], TINY_BATCH[1], 80, lengths=TINY_BATCH[2], seed=11)
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=args.vocab_size)
    lm_state = synth.make_state(lm_args, seed=9, gain=2.0)
    return args, state, feats, sizes, lm_args, lm_state, dict(extra or {})


def _config2():
    args = synth.make_args("config2", decode_type="ctc_only", ctc_lm_weight=0.1, ctc_beam=5, ctc_pruning=8, ctc_lp=0.5, lm_weight=0)
    state = synth.make_state(args, seed=0, blank_bias=0.35)
    feats, sizes = synth.make_feats(2, 300, 80, lengths=[300, 231], seed=11)
    lm_args = synth.make_args_lm("lm_small", vocab_size=args.vocab_size)
    return args, state, feats, sizes, lm_args, synth.make_state(lm_args, seed=9), {}


CASES = {
    "ctc_lm_tiny": lambda: _tiny(seed=2),
    "ctc_lm_tiny_b1": lambda: _tiny(seed=2, ctc_beam=1),
    "ctc_lm_tiny_lp0": lambda: _tiny(seed=2, ctc_lm_weight=0.1, ctc_lp=0.0),
    # a blank bias: utterance 0 skips a frame (blank probability above 0.95) that the other two utterances process
    "ctc_lm_tiny_skip": lambda: _tiny(seed=3, blank_bias=4.0, extra=dict(needs_skip=True)),
    "ctc_lm_tiny_ctcatt": lambda: _tiny(seed=3, decode_type="ctc_att", sample_num=1, beam_width=1, extra=dict(ctc_att=True)),
    "ctc_lm_tiny_conf": lambda: _tiny(preset="tiny_conf", seed=2),
    "ctc_lm_config2": _config2,
}

TINY = [n for n in CASES if n != "ctc_lm_config2"]
