"""The conformer AST model (src/models/conformer.py) on the host side: checkpoint names and shapes, the task wiring, the
refusals, and the C ABI's definition of ast = 1 with the conformer flags.  No GPU needed."""
import ctypes as C
from types import SimpleNamespace

import pytest

from cassnat_asr_public_amd import hip, synth


def shapes_of(model):
    return {k: tuple(p.shape) for k, p in model.named_parameters()}


@pytest.mark.parametrize("preset,over", [("tiny_conf_ast", {}), ("config4_conf", {}), ("tiny_conf_ast", dict(interctc_alpha=0.5))])
def test_make_conformer_has_the_reference_checkpoint_names_and_shapes(preset, over):
    from cassnat_asr_public_amd.models import make_conformer

    args = synth.make_args_ast(preset, **over)
    model = make_conformer(args.input_size, args)
    want = synth.param_shapes_conformer_ast(args)
    assert list(dict(model.named_parameters())) == list(want)  # (registration order = the reference's)
    assert shapes_of(model) == dict(want)
    assert ("interctc_generator.norm.a_2" in want) == (over.get("interctc_alpha", 0) > 0)
    hy = model._hyper
    assert (hy["ast"], hy["conf_enc"], hy["enc_max_rel"], hy["enc_kernel"]) == (1, 1, args.enc_max_relative_len, args.enc_kernel_size)
    assert (hy["d_encff"], hy["d_decff"], hy["N_mix_dec"]) == (args.d_encff, args.d_decff, args.N_dec)
    # the position rows are the frozen sinusoid table, not re-initialised
    import numpy as np

    np.testing.assert_allclose(model.src_embed.pos_enc.embedding.weight.numpy(),
                               synth.sinusoid_rows(args.d_model, 2 * args.enc_max_relative_len + 1), atol=1e-5)


def test_synth_state_of_the_conformer_ast_follows_its_shapes():
    args = synth.make_args_ast("tiny_conf_ast")
    state = synth.make_state(args, seed=3)
    assert {k: v.shape for k, v in state.items()} == dict(synth.param_shapes_conformer_ast(args))
    # the transformer AST's seeded state is what it always was
    a = synth.make_args_ast("tiny_ast")
    assert list(synth.make_state(a, seed=3)) == list(synth.param_shapes_ast(a))


def test_art_task_builds_the_conformer_model():
    from cassnat_asr_public_amd.models.conformer import Conformer
    from cassnat_asr_public_amd.tasks.art_task import ArtTask

    args = synth.make_args_ast("tiny_conf_ast", model_type="conformer")
    task = SimpleNamespace()
    ArtTask.set_model(task, args)
    assert isinstance(task.model, Conformer)
    args = synth.make_args_ast("tiny_ast", model_type="transformer")
    ArtTask.set_model(task, args)
    assert type(task.model).__name__ == "Transformer"
    with pytest.raises(NotImplementedError, match="knows transformer, conformer"):
        ArtTask.set_model(task, synth.make_args_ast("tiny_ast", model_type="lstm"))


@pytest.mark.parametrize("over,msg", [(dict(pos_type="absolute"), "convolution module before self attention"),
                                      (dict(share_ff=True), "share_ff")])
def test_unsupported_conformer_variants_are_refused(over, msg):
    from cassnat_asr_public_amd.models.conformer import make_model

    args = synth.make_args_ast("tiny_conf_ast", **over)
    with pytest.raises(NotImplementedError, match=msg):
        make_model(args.input_size, args)


def test_fp8_request_runs_the_conformer_ast_in_bf16():
    from cassnat_asr_public_amd.models.conformer import make_model

    args = synth.make_args_ast("tiny_conf_ast", hip_precision="fp8")
    assert make_model(args.input_size, args).hip_precision == "bf16"


def test_swish_entry_points_are_declared_and_exported():
    names = hip.declared_symbols()
    for name in ("cn_op_ffn_fused_act", "cn_op_ffn_x3_act"):
        assert name in names
        getattr(hip.lib(), name)
        getattr(hip.lib("f16"), name)


@pytest.mark.parametrize("flags", [dict(ast=1, conf_dec=1), dict(ast=1, conf_enc=1, conf_dec=1), dict(ast=2, conf_enc=1)])
def test_model_create_refuses_conformer_combinations_the_reference_does_not_define(flags):
    """ast = 1 with conf_enc is the conformer AST; a conformer DECODER under the AST (or a conformer TransformerLM) does not
    exist in the reference and must not silently build something else.  (Refused before any device is touched.)"""
    L = hip.lib()
    cfg = hip.CnConfig(input_size=80, d_model=128, n_head=2, d_encff=256, d_decff=256, n_enc=2, n_extra=0, n_self_dec=0, n_mix_dec=2,
                       vocab_size=40, precision=hip.PRECISION["fp32"], max_batch=2, max_frames=64, device=0, enc_max_rel=5,
                       dec_max_rel=3, enc_kernel=7, dec_kernel=3, **flags)
    h = C.c_void_p()
    rc = L.cn_model_create(C.byref(cfg), C.byref(h))
    assert rc != 0 and not h.value
    assert b"conformer" in L.cn_last_error()
