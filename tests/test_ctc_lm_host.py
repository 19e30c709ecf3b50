"""CTC prefix beam search with in-loop LM fusion, the parts that need no GPU: the C ABI (declared and exported by both libraries,
null arguments refused before any launch), ctc_beam_decode's refusal of anything but a TransformerLM, the task keeping such runs
off the pipelined path and the refusals that stay."""
from types import SimpleNamespace

import pytest

from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models import make_cassnat_model
from cassnat_asr_public_amd.models.lm import TransformerLM
from cassnat_asr_public_amd.tasks.cassnat_task import CassNATTask
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode

NEW = ("cn_ctc_beam_lm", "cn_lm_step_rows", "cn_op_ctc_lm_frame", "cn_op_ctc_lm_rows")


def test_entry_points_are_declared_and_exported_by_both_libraries():
    names = hip.declared_symbols()
    for name in NEW:
        assert name in names
        assert getattr(hip.lib(), name).argtypes is not None
        assert getattr(hip.lib("f16"), name).argtypes is not None


@pytest.mark.parametrize("flavour", [None, "f16"])
def test_null_arguments_are_refused_before_any_launch(flavour):
    L = hip.lib(flavour)
    assert L.cn_ctc_beam_lm(None, None, None, None, 2, 61, 80, None, 5, 8, 0.2, 0.3, None, 17, None, None, None, None, None, None, None, None) != 0
    assert L.cn_last_error()  # (the model handle is checked first, as in cn_ctc_beam)
    assert L.cn_lm_step_rows(None, 4, 0, None, None, None, None, 4, None, None) != 0
    assert b"cn_lm_step_begin first" in L.cn_last_error()
    assert L.cn_op_ctc_lm_frame(*([None] * 20), 2, 4, 40, 3, 5, 0, 1, 0, 6, 4, 0.0, 0.3, None) != 0
    assert b"null array" in L.cn_last_error()
    assert L.cn_op_ctc_lm_rows(None, None, None, None, None, None, 0, 6, 3, 40, None) != 0
    assert b"null array" in L.cn_last_error()


@pytest.mark.parametrize("lm_model", [object(), SimpleNamespace(teacher_score=lambda *a: None), SimpleNamespace(score=lambda text: 0.0)])
def test_anything_but_a_transformer_lm_is_refused_before_vocab_or_args_are_touched(lm_model):
    """An at_baseline ranker (teacher_score) or an n-gram model (score) in lm_model ends in the refusal, not in an attribute error."""
    with pytest.raises(NotImplementedError, match="in-loop LM fusion"):
        ctc_beam_decode(None, None, None, None, None, None, lm_model)


@pytest.mark.parametrize("decode_type", ["ctc_only", "ctc_att"])
def test_decode_keeps_ctc_lm_runs_off_the_pipelined_path(tmp_path, decode_type):
    task = object.__new__(CassNATTask)
    calls = []
    task.test_loader, task.world, task.rank = [0, 1, 2], 1, 0
    task._decode_pipelined = lambda *a: calls.append("pipelined") or (0, -1)
    task._decode_plain = lambda *a: calls.append("plain") or (0, -1)
    scp = tmp_path / "feats.scp"
    scp.write_text("")
    args = SimpleNamespace(beam_width=1, sample_num=1, decode_type=decode_type, lm_weight=0, ctc_lm_weight=0.3, hip_pipelines=2, print_freq=1,
                           test_paths=[{"scp_path": str(scp)}], result_file=str(tmp_path / "out.txt"), print_utt2diff=False)
    task.decode(args)
    assert calls == ["plain"]


def test_refusals_that_stay():
    from cassnat_asr_public_amd.tasks.art_task import ArtTask

    lm = TransformerLM(synth.make_args_lm("tiny_lm", vocab_size=40))
    args = synth.make_args("tiny", decode_type="ctc_att", sample_num=4, ctc_lm_weight=0.3)
    model = make_cassnat_model(args.input_size, args)
    with pytest.raises(NotImplementedError, match="ctc_att with sample_num > 1"):
        model._check_args(args, lm)
    with pytest.raises(NotImplementedError, match="in-loop LM fusion"):
        ArtTask.load_lm_model(SimpleNamespace(lm_model=None), SimpleNamespace(ctc_lm_weight=0.3, decode_type="ctc_only", lm_weight=0))
