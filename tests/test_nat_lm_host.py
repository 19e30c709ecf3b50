"""CASS-NAT decoding with LM shallow fusion, the parts that need no GPU: CassNATTask.load_lm_model with lm_weight > 0
(src/tasks/cassnat_task.py:85-127), the refusals that stay, decode() keeping such runs off the pipelined path, and the C ABI."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch
import yaml

from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models import make_cassnat_model
from cassnat_asr_public_amd.models.lm import TransformerLM
from cassnat_asr_public_amd.tasks.cassnat_task import CassNATTask


def _lm_files(tmp_path, prefix="", key="model_state"):
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=40)
    state = synth.make_state(lm_args, seed=9, gain=2.0)
    conf = tmp_path / "lm.yaml"
    conf.write_text(yaml.safe_dump({k: getattr(lm_args, k) for k in ("d_model", "n_head", "d_ff", "N", "dropout")}))
    ckpt = tmp_path / "lm.mdl"
    torch.save({key: {prefix + k: torch.from_numpy(v) for k, v in state.items()}}, str(ckpt))
    return str(conf), str(ckpt), state


def _task():
    return SimpleNamespace(vocab=SimpleNamespace(n_words=40), lm_model=None)


def _args(conf, ckpt, **over):
    d = dict(lm_weight=0.6, ctc_lm_weight=0, rank_model="lm", lm_config=conf, rnnlm=ckpt, hip_precision="fp32", input_size=80)
    d.update(over)
    return SimpleNamespace(**d)


@pytest.mark.parametrize("prefix", ["", "module."])
def test_load_lm_model_with_lm_weight(tmp_path, prefix):
    conf, ckpt, state = _lm_files(tmp_path, prefix)
    task = _task()
    CassNATTask.load_lm_model(task, _args(conf, ckpt))
    lm = task.lm_model
    assert isinstance(lm, TransformerLM)
    assert lm.hip_precision == "fp32" and lm.out_generator.proj.weight.shape == (40, 128)  # the model's precision is inherited
    for k, p in lm.named_parameters():
        assert torch.equal(p.detach(), torch.from_numpy(state[k])), k


def test_load_lm_model_reads_the_model_state_key(tmp_path):
    conf, ckpt, _ = _lm_files(tmp_path, key="state_dict")
    with pytest.raises(KeyError):
        CassNATTask.load_lm_model(_task(), _args(conf, ckpt))


def test_lm_weight_zero_still_gives_no_lm():
    task = _task()
    CassNATTask.load_lm_model(task, SimpleNamespace(lm_weight=0, ctc_lm_weight=0, rank_model="lm", lm_config=None, rnnlm=None))
    assert task.lm_model is None


@pytest.mark.parametrize("rank", ["at_baseline", "n-gram"])
def test_load_lm_model_refuses_the_other_rankers_with_lm_weight(tmp_path, rank):
    conf, ckpt, _ = _lm_files(tmp_path)
    with pytest.raises(NotImplementedError, match="rank_model 'lm'"):
        CassNATTask.load_lm_model(_task(), _args(conf, ckpt, rank_model=rank, ctc_lm_weight=0.5))


def _model(**over):
    args = synth.make_args("tiny", **over)
    return make_cassnat_model(args.input_size, args), args


def test_lm_weight_without_an_lm_is_a_value_error():
    model, args = _model(lm_weight=0.6, beam_width=3)
    with pytest.raises(ValueError, match="lm_model"):
        model._check_args(args, None)


def test_refusals_that_stay():
    lm = TransformerLM(synth.make_args_lm("tiny_lm", vocab_size=40))
    ranker = SimpleNamespace(teacher_score=lambda *a: None)   # what an at_baseline ranker offers
    ngram = SimpleNamespace(score=lambda text: 0.0)
    model, args = _model(lm_weight=0.6, beam_width=3, sample_num=4, rank_model="at_baseline")
    with pytest.raises(NotImplementedError, match="at_baseline"):
        model._check_args(args, ranker)
    args.rank_model = "n-gram"
    with pytest.raises(NotImplementedError, match="n-gram"):
        model._check_args(args, ngram)
    model, args = _model(lm_weight=0.6, beam_width=3)
    with pytest.raises(NotImplementedError, match="TransformerLM"):
        model._check_args(args, ranker)                        # not a TransformerLM: nothing to fuse
    model, args = _model(lm_weight=0.6, beam_width=17)
    with pytest.raises(NotImplementedError, match="beam_width"):
        model._check_args(args, lm)
    model, args = _model(lm_weight=0.6, beam_width=3, decode_type="ctc_att", sample_num=4)
    with pytest.raises(NotImplementedError, match="ctc_att with sample_num > 1"):
        model._check_args(args, lm)
    model, args = _model(lm_weight=0.6, beam_width=3, test_hitrate=True)
    with pytest.raises(NotImplementedError, match="test_hitrate"):
        model._check_args(args, lm)
    for ok in (dict(), dict(beam_width=1), dict(use_trigger=False), dict(decode_type="ctc_att", sample_num=1),
               dict(sample_num=4, rank_model="lm")):
        model, args = _model(**dict(dict(lm_weight=0.6, beam_width=3), **ok))
        model._check_args(args, lm)                            # in scope now


@pytest.mark.parametrize("lm_weight,pipelined", [(0.3, False), (0, True)])
def test_decode_keeps_lm_fusion_off_the_pipelined_path(tmp_path, lm_weight, pipelined):
    """beam_width 1 with lm_weight > 0 is not the greedy finish: the decode pipelines would silently drop the LM."""
    task = object.__new__(CassNATTask)
    calls = []
    task.test_loader, task.world, task.rank = [0, 1, 2], 1, 0
    task._decode_pipelined = lambda *a: calls.append("pipelined") or (0, -1)
    task._decode_plain = lambda *a: calls.append("plain") or (0, -1)
    scp = tmp_path / "feats.scp"
    scp.write_text("")
    args = SimpleNamespace(beam_width=1, sample_num=0, decode_type="att_only", lm_weight=lm_weight, hip_pipelines=2, print_freq=1,
                           test_paths=[{"scp_path": str(scp)}], result_file=str(tmp_path / "out.txt"), print_utt2diff=False)
    assert task.decode(args) == 0
    assert calls == ["pipelined" if pipelined else "plain"]


def test_decode_opts_layout_is_unchanged():
    """The keep-rows flag lives in reserved[0]: the struct's size and every offset stay what C callers compiled against."""
    assert C.sizeof(hip.CnDecodeOpts) == 64
    names = ["padding_idx", "sos", "left_trigger", "right_trigger", "src_trigger", "use_unimask", "beam_width", "capture", "sub_batch",
             "no_trigger"]
    for i, n in enumerate(names):
        assert getattr(hip.CnDecodeOpts, n).offset == 4 * i and getattr(hip.CnDecodeOpts, n).size == 4
    assert hip.CnDecodeOpts.reserved.offset == 40 and hip.CnDecodeOpts.reserved.size == 24
    assert list(hip.Engine.make_opts(synth.make_args("tiny", lm_weight=0.6)).reserved) == [0] * 6


def test_entry_points_are_declared_and_exported():
    names = hip.declared_symbols()
    for name in ("cn_nat_attach_lm", "cn_nat_lm_finish", "cn_op_nat_lm_fuse_topk", "cn_op_nat_beam_update"):
        assert name in names
        getattr(hip.lib(), name)
        getattr(hip.lib("f16"), name)


def test_attach_and_finish_refuse_null_handles():
    """Null handles and arrays are refused before anything else (the geometry refusals of the kernel entries run on real
    allocations in tests/test_gpu_nat_lm_kernels.py)."""
    L = hip.lib()
    assert L.cn_nat_attach_lm(None, None) != 0
    assert b"cfg.ast = 0" in L.cn_last_error()
    assert L.cn_nat_lm_finish(None, None, 3, 3, 0.5, 1, 0.0, 0, None, 4, None, None, None) != 0
    assert b"null argument" in L.cn_last_error()
    assert L.cn_op_nat_lm_fuse_topk(None, None, None, None, 2, 5, 40, 3, 0, 0.5, 3, None, None, None) != 0
    assert b"bad argument" in L.cn_last_error()
    assert L.cn_op_nat_beam_update(*([None] * 12), 0, 0, 3, 8, 0, 1, 0.0, 2, None) != 0
    assert b"null array" in L.cn_last_error()


@pytest.mark.parametrize("decode_type", ["ctc_att", "ctc_only"])
@pytest.mark.parametrize("ctc_lm_weight", [0, 0.2])
def test_plain_loop_hands_the_fused_lm_to_beam_decode_only(decode_type, ctc_lm_weight, monkeypatch):
    """With lm_weight > 0 the task holds a TransformerLM.  ctc_beam_decode gets it only when ctc_lm_weight > 0, as the reference's
    reads it only then (this package's refuses any lm_model); beam_decode always gets it - so `decode_type: ctc_att` with
    --lm_weight runs through CassNATTask."""
    from cassnat_asr_public_amd.tasks import cassnat_task

    lm, seen = object(), {}

    def fake_ctc(model, feats, mask, sizes, vocab, args, lm_model):
        seen["ctc"] = lm_model
        return "top"

    def fake_beam(feats, mask, sizes, vocab, args, lm_model, top=None, labels=None, label_sizes=None):
        seen["beam"] = (lm_model, top)
        return [[{"hyp": [1, 5, 2]}]], args

    monkeypatch.setattr(cassnat_task, "ctc_beam_decode", fake_ctc)
    task = object.__new__(CassNATTask)
    task.model = SimpleNamespace(eval=lambda: None, beam_decode=fake_beam)
    task.lm_model, task.rank = lm, 0
    task.vocab = SimpleNamespace(word2index={"sos": 1, "eos": 2}, index2word={5: "w"})
    task.test_loader = [(["u0"], torch.ones(1, 8, 80), torch.zeros(1, 2, dtype=torch.long), torch.ones(1), torch.tensor([2]))]
    args = SimpleNamespace(padding_idx=0, decode_type=decode_type, lm_weight=0.6, ctc_lm_weight=ctc_lm_weight, print_freq=100)
    results = {}
    if decode_type == "ctc_only":
        monkeypatch.setattr(cassnat_task, "ctc_beam_decode", lambda *a: seen.__setitem__("ctc", a[-1]) or [[{"hyp": [5]}]])
    task._decode_plain(args, results, SimpleNamespace(update=lambda t: None), SimpleNamespace(print=lambda i: None))
    assert seen["ctc"] is (lm if ctc_lm_weight > 0 else None)
    if decode_type == "ctc_att":
        assert seen["beam"] == (lm, "top")
    assert results["u0"][0] == ["w"]
