"""Packed decoder rows: a greedy pass of the row-chain engines gives every utterance only the rows its hypothesis
reads, one utterance behind the other, instead of U rows each.  The padded layout stays in the library behind
``cn_decode_opts.reserved[1]`` (``args.hip_padded_rows``); hypotheses, lengths and float64 scores of the two layouts must be
EQUAL - the padded rows were never read, and a key past an utterance's own rows gives the bits a masked key gave."""
import numpy as np
import pytest
import torch

import packed_cases as pc
from cassnat_asr_public_amd.models.cassnat import make_model
from oracle import cassnat_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    args, state, feats, sizes = pc.make_case()
    ref = orc.decode_nast(state, feats, sizes, args, stages=True)
    total = pc.check_row_counts(ref["ylen"])
    return dict(args=args, state=state, feats=feats, sizes=sizes, ref=ref, total=total, models={})


def model_of(case, prec):
    if prec not in case["models"]:
        args = case["args"]
        args.hip_precision, args.hip_capture = prec, False
        model = make_model(args.input_size, args).cuda()
        with torch.no_grad():
            for k, p in model.named_parameters():
                p.copy_(torch.from_numpy(case["state"][k]))
        case["models"][prec] = model
    case["args"].hip_precision = prec
    return case["models"][prec]


def both_layouts(case, prec, feats, sizes, **kw):
    """The same call on packed and on padded decoder rows -> ((hyp, hyp_len, score) numpy, per layout), ylen, ymax."""
    model, args = model_of(case, prec), case["args"]
    got = []
    for padded in (False, True):
        args.hip_padded_rows = padded
        out = model.decode_device(torch.from_numpy(feats), torch.from_numpy(sizes), args, 1, **kw)
        torch.cuda.synchronize()
        got.append(tuple(t.cpu().numpy() for t in out[:3]))
    args.hip_padded_rows = False
    eng = model._engine
    return got[0], got[1], eng.fetch("ylen"), int(eng.fetch("ymax")[0])


def assert_equal_layouts(packed, padded, what):
    for name, a, b in zip(("hyp", "hyp_len", "score"), packed, padded):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert np.isfinite(a.astype(np.float64)).all(), (what, name)
        assert (a == b).all(), (what, name, np.argwhere(a != b)[:4].tolist())


def hyps_of(out):
    hyp, hyp_len, _ = out
    return [hyp[b, : hyp_len[b]].tolist() for b in range(hyp.shape[0])]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_plain_pass(case, prec):
    """bf16, and once through the half-precision library."""
    packed, padded, ylen, ymax = both_layouts(case, prec, case["feats"], case["sizes"])
    assert_equal_layouts(packed, padded, "plain")
    ref = case["ref"]
    # the row counts are integer work on the arg-max path: where the engine's path is the oracle's, so are they - and the
    # hypotheses have the oracle's lengths (the padded-path tests of the 16-bit engines ask no token-for-token agreement)
    if (model_of(case, prec)._engine.fetch("best_paths") == np.asarray(ref["best_paths"])).all():
        np.testing.assert_array_equal(ylen, np.asarray(ref["ylen"]))
        assert [len(h) for h in hyps_of(packed)] == [len(h) for h in ref["hyps"]]
    # the engine's own counts meet the conditions the inputs were chosen for
    pc.check_row_counts(ylen)
    assert packed[1].tolist() == (pc.rows_read(ylen) + 1).tolist()


def test_fetching_packed_token_rows_is_refused(case):
    from cassnat_asr_public_amd import hip

    both_layouts(case, "bf16", case["feats"], case["sizes"])
    model, args = model_of(case, "bf16"), case["args"]
    model.decode_device(torch.from_numpy(case["feats"]), torch.from_numpy(case["sizes"]), args, 1)
    with pytest.raises(hip.HipError, match="packed"):
        model._engine.fetch("tok")
    args.hip_padded_rows = True
    model.decode_device(torch.from_numpy(case["feats"]), torch.from_numpy(case["sizes"]), args, 1)
    args.hip_padded_rows = False
    assert model._engine.fetch("tok").shape[0] == len(pc.LENGTHS)


def test_sub_batch_of_two_batches(case):
    """Two coalesced batches of four: the second batch's utterances are limited by ITS largest count (23 rows, not 73)."""
    packed, padded, ylen, _ = both_layouts(case, "bf16", case["feats"], case["sizes"], sub_batch=4)
    assert_equal_layouts(packed, padded, "sub_batch")
    want = np.concatenate([pc.rows_read(ylen[:4]), pc.rows_read(ylen[4:])])
    assert packed[1].tolist() == (want + 1).tolist()
    assert int(want[4]) < int(ylen[4]) + 1  # (the limit of the utterance's own batch binds)
    # and each batch is what a pass of its own gives
    for k in range(2):
        alone, _, _, _ = both_layouts(case, "bf16", case["feats"][4 * k: 4 * k + 4], case["sizes"][4 * k: 4 * k + 4])
        n = alone[0].shape[1]
        assert (alone[0] == packed[0][4 * k: 4 * k + 4, :n]).all() and (alone[2] == packed[2][4 * k: 4 * k + 4]).all(), k


def test_merged_pass_of_two_frame_counts(case):
    feats, sizes, rows, frames, parts = pc.make_merged_case()
    packed, padded, _, _ = both_layouts(case, "bf16", feats, sizes, sub_rows=rows, sub_frames=frames)
    assert_equal_layouts(packed, padded, "merged")
    lo = 0
    for k, (f, s) in enumerate(parts):
        alone, _, _, _ = both_layouts(case, "bf16", f, s)
        n = min(alone[0].shape[1], packed[0].shape[1])
        assert hyps_of(alone) == hyps_of(tuple(t[lo: lo + rows[k]] for t in packed)), k
        assert (alone[2] == packed[2][lo: lo + rows[k]]).all(), k
        assert n > 0
        lo += rows[k]


@pytest.mark.parametrize("hint", ["frames", "exact"])
def test_predicted_row_count(case, hint):
    """U = T' + 1 (101 rows of capacity per utterance, 73 used at most: whole workgroups of every row kernel leave at once)
    and U = the true maximum; both must equal the exact pass."""
    exact, exact_padded, ylen, ymax = both_layouts(case, "bf16", case["feats"], case["sizes"])
    assert_equal_layouts(exact, exact_padded, "exact")
    U = pc.subsampled(case["feats"].shape[1]) + 1 if hint == "frames" else ymax
    assert U >= ymax
    if hint == "frames":  # the capacity holds whole 128-row workgroups behind the rows that exist
        assert (len(pc.LENGTHS) * U + 127) // 128 > (int(pc.rows_read(ylen).sum()) + 127) // 128 + 1
    model, args = model_of(case, "bf16"), case["args"]
    got = []
    for padded in (False, True):
        args.hip_padded_rows = padded
        hyp, hyp_len, score, t = model.decode_device(torch.from_numpy(case["feats"]), torch.from_numpy(case["sizes"]), args, 1,
                                                     u_hint=U, want_ticket=True)
        torch.cuda.synchronize()
        assert model._engine.ticket(t) == (ymax, U)
        got.append((hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy()))
    args.hip_padded_rows = False
    assert_equal_layouts(got[0], got[1], hint)
    assert hyps_of(got[0]) == hyps_of(exact) and (got[0][2] == exact[2]).all()
