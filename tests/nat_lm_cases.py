"""The seeded inputs of the CASS-NAT + LM fixtures (tools/make_nat_lm_goldens.py writes them from the reference's own
CassNAT.beam_decode with lm_weight > 0; tests/test_nat_lm_model.py and tests/test_gpu_nat_lm.py read them).  Every case returns
(args, state, feats, sizes, lm_args, lm_state, extra): ``extra`` holds what the generator needs beside them (the seed of the
ESA draws, the CTC beam options)."""
from cassnat_asr_public_amd import synth

TINY_BATCH = (3, 61, [61, 50, 37])


def _tiny(preset="tiny", seed=0, extra=None, **ov):
    ov.setdefault("beam_width", 3)
    ov.setdefault("lm_weight", 0.6)
    ov.setdefault("length_penalty", 0.1)
    args = synth.make_args(preset, **ov)
    state = synth.make_state(args, seed=seed, gain=2.0)
    feats, sizes = synth.make_feats(TINY_BATCH[0], TINY_BATCH[1], 80, lengths=TINY_BATCH[2], seed=11)
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=args.vocab_size)
    lm_state = synth.make_state(lm_args, seed=9, gain=2.0)
    return args, state, feats, sizes, lm_args, lm_state, dict(extra or {})


def _config2():
    args = synth.make_args("config2", beam_width=5, lm_weight=0.3, length_penalty=0)
    state = synth.make_state(args, seed=0, blank_bias=0.35)
    feats, sizes = synth.make_feats(2, 300, 80, lengths=[300, 231], seed=11)
    lm_args = synth.make_args_lm("lm_small", vocab_size=args.vocab_size)
    return args, state, feats, sizes, lm_args, synth.make_state(lm_args, seed=9), {}


CASES = {
    # seed 2: kept beams hold token 0 inside the prefix, so the LM key mask (ys != padding_idx) is exercised
    "nat_lm_tiny": lambda: _tiny(seed=2, extra=dict(needs_blank=True)),
    "nat_lm_tiny_bw1": lambda: _tiny(beam_width=1, lm_weight=0.3),
    "nat_lm_tiny_esa": lambda: _tiny(sample_num=4, threshold=0.9, rank_model="lm", lm_weight=0.4, length_penalty=0,
                                     extra=dict(select_seed=5)),
    "nat_lm_tiny_ctcatt": lambda: _tiny(decode_type="ctc_att", sample_num=1, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0,
                                        extra=dict(ctc_att=True)),
    "nat_lm_tiny_notrigger": lambda: _tiny(use_trigger=False),
    "nat_lm_tiny_conf": lambda: _tiny(preset="tiny_conf", seed=4),
    "nat_lm_config2": _config2,
}

TINY = [n for n in CASES if n != "nat_lm_config2"]
# the tiny cases whose fixture carries the reference's att_out (no ESA: its att_out is masked and gathered per sample)
WITH_ATT_OUT = [n for n in TINY if n != "nat_lm_tiny_esa"]
