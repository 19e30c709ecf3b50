"""The restatement of the fused finish loop (tests/nat_lm_model.py) against the reference's own beams: on the reference's att_out
of every tiny fixture that carries one, with the float32 oracle of the TransformerLM as the LM, it must reproduce every beam.
That pins the model the kernel tests (tests/test_gpu_nat_lm_kernels.py) compare the device against.  No GPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from nat_lm_cases import CASES, WITH_ATT_OUT
from nat_lm_model import beam_step, fused_finish, fused_row_topk, init_state
from oracle import cassnat_oracle as orc


def oracle_lm(lm_args, lm_state):
    st = orc.to_torch_state(lm_state)

    def lm(ys, mask):
        with torch.no_grad():
            return orc.lm_forward(st, torch.from_numpy(ys).long(), torch.from_numpy(mask), lm_args.N, lm_args.n_head)[:, -1].numpy()
    return lm


@pytest.mark.parametrize("name", WITH_ATT_OUT)
def test_model_reproduces_every_reference_beam(name):
    g = load_golden(name)
    args, _, _, _, lm_args, lm_state, _ = CASES[name]()
    att_out = g["att_out"]
    beams = fused_finish(att_out, g["ylen"], att_out.shape[1], oracle_lm(lm_args, lm_state), args.beam_width, args.lm_weight,
                         args.length_penalty)
    for b, utt in enumerate(beams):
        assert len(utt) == g["beam_hyp"].shape[1]
        for j, s in enumerate(utt):
            assert s["hyp"] == g["beam_hyp"][b, j, : g["beam_len"][b, j]].tolist(), (b, j)
            assert abs(s["score"] - g["beam_score"][b, j]) < max(5e-3, 1e-6 * abs(g["beam_score"][b, j]))


def test_the_lm_changes_the_best_hypothesis():
    """A decode that ignores the LM cannot match the fixture: at lm_weight 0 the best beam of every utterance differs."""
    g = load_golden("nat_lm_tiny")
    args, _, _, _, lm_args, lm_state, _ = CASES["nat_lm_tiny"]()
    att_out = g["att_out"]
    V = att_out.shape[2]
    beams = fused_finish(att_out, g["ylen"], att_out.shape[1], lambda ys, mask: np.zeros((ys.shape[0], V), np.float32), args.beam_width,
                         args.lm_weight, args.length_penalty)
    assert all(utt[0]["hyp"] != g["beam_hyp"][b, 0, : g["beam_len"][b, 0]].tolist() for b, utt in enumerate(beams))


def test_the_tiny_fixture_holds_a_blank_inside_a_kept_prefix():
    g = load_golden("nat_lm_tiny")
    assert any(0 in g["beam_hyp"][b, j, 1: g["beam_len"][b, j] - 1] for b in range(3) for j in range(3))


def test_fused_row_ties_go_to_the_lower_index():
    att = np.zeros(8, np.float32)
    lm = np.array([-1, -3, -1, -2, -1, -9, -9, -9], np.float32)
    idx, val = fused_row_topk(att, lm, 0.5, 4)
    assert idx.tolist() == [0, 2, 4, 3] and val.tolist() == [-0.5, -0.5, -0.5, -1.0]


def test_beam_step_keeps_list_order_on_tied_keys_and_carries_ended_utterances():
    bw = 2
    st = init_state(2, bw, 5)
    idx = np.array([[5, 6], [7, 8], [9, 10], [11, 12]], np.int32)
    val = np.full((4, 2), -1.0, np.float32)
    st1 = beam_step(st, idx, val, np.array([2, -1]), 0, bw)
    assert st1["tok"][0, :2].tolist() == [1, 5] and st1["tok"][1, :2].tolist() == [1, 6]   # step 0: one live beam, list order
    assert st1["tok"][2:].tolist() == st["tok"][2:].tolist() and st1["score"][2:].tolist() == [0.0, 0.0]  # utterance 1 ended
    st2 = beam_step(st1, idx, val, np.array([2, -1]), 1, bw, length_penalty=None)
    assert st2["tok"][0, :3].tolist() == [1, 5, 5] and st2["tok"][1, :3].tolist() == [1, 5, 6]  # four tied keys: the first two
    assert st2["anc"][1, :3].tolist() == [0, 0, 1] and st2["score"][:2].tolist() == [-2.0, -2.0]
    st3 = beam_step(st2, np.zeros((4, 2), np.int32), val, np.array([2, -1]), 2, bw)
    assert st3["keyok"][0, :4].tolist() == [1, 1, 1, 0]  # a blank inside the prefix is masked for later positions
