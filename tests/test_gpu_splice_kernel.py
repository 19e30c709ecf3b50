"""cn_op_splice_rows against the host definition (``speech_loader.splice_host``: the dataset's CMVN in float64, zero rows up to a
multiple of skip, ``feat_op.context_feat`` / ``skip_feat``; then collate's padding), bit for bit: both calling forms - packed
archive rows with statistics, a padded normalised batch without -, the 16-byte and the scalar path, every chunk boundary, the
clamps and the refusals."""
import numpy as np
import pytest
import torch

from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.data.speech_loader import splice_host

pytestmark = pytest.mark.gpu

TRIPLES = [(0, 2, 1), (1, 1, 2), (3, 0, 1), (0, 0, 3), (2, 2, 3), (0, 0, 1)]
LENGTHS = [1, 31, 32, 33, 64, 65, 7]  # around the 32-frame chunk; the last is shorter than its neighbours' T_out
PAD = 7.0

_cache = {}


def case(F0):
    """Matrices, statistics whose mean is far from 0 (a zero row normalised by mistake would be about -12 / std), and the packed
    source: the utterances one after the other behind five leading rows, a row of NaN between any two (a read past an utterance's
    own rows shows)."""
    if F0 not in _cache:
        rng = np.random.default_rng(100 + F0)
        mats = [(rng.standard_normal((n, F0)) * 2.5 + 9.0).astype(np.float32) for n in LENGTHS]
        mean, std = rng.standard_normal(F0) * 3 + 12, rng.random(F0) + 0.5
        offs, parts, o = [], [np.full((5, F0), np.nan, np.float32)], 5
        for m in mats:
            offs.append(o)
            parts += [m, np.full((1, F0), np.nan, np.float32)]
            o += m.shape[0] + 1
        _cache[F0] = (mats, (mean, std), np.vstack(parts), offs)
    return _cache[F0]


def expected(mats, triple, T_out, cmvn=None):
    blocks = triple[0] + triple[1] + 1
    out = np.full((len(mats), T_out, blocks * mats[0].shape[1]), PAD, np.float32)
    for b, m in enumerate(mats):
        s = splice_host(m, triple, cmvn)
        n = min(s.shape[0], T_out)
        out[b, :n] = s[:n]  # (one rounding to float32, as collate's)
    return out


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device="cuda")


def run(src, offs, lens, triple, T_out, F0, cmvn=None):
    blocks = triple[0] + triple[1] + 1
    out = torch.full((len(lens), T_out, blocks * F0), -3.0, device="cuda")
    stats = (None, None) if cmvn is None else (torch.from_numpy(cmvn[0]).cuda(), torch.from_numpy(cmvn[1]).cuda())
    hip.splice_rows(src, i32(offs), i32(lens), out, triple[0], triple[1], triple[2], PAD, stats[0], stats[1])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def n_out(n, skip):
    return -(-n // skip) if skip > 1 else n


@pytest.mark.parametrize("with_cmvn", [False, True])
@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "%d-%d-%d" % t)
@pytest.mark.parametrize("F0", [80, 83, 4])
def test_splice_rows_is_the_datasets_splice_on_the_device(F0, triple, with_cmvn):
    mats, cmvn, packed, offs = case(F0)
    cmvn = cmvn if with_cmvn else None
    T_out = n_out(max(LENGTHS), triple[2]) + 3  # every utterance is shorter than T_out: pad rows behind each
    src = torch.from_numpy(packed).cuda()
    got = run(src, offs, LENGTHS, triple, T_out, F0, cmvn)
    want = expected(mats, triple, T_out, cmvn)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, want)
    if triple == (0, 0, 1):  # the unspliced form is cn_op_unpack_rows
        out = torch.full((len(LENGTHS), T_out, F0), -3.0, device="cuda")
        stats = (None, None) if cmvn is None else (torch.from_numpy(cmvn[0]).cuda(), torch.from_numpy(cmvn[1]).cuda())
        hip.unpack_rows(src, i32(offs), i32(LENGTHS), out, PAD, stats[0], stats[1])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got, out.cpu().numpy())


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "%d-%d-%d" % t)
@pytest.mark.parametrize("F0", [80, 83])
def test_second_calling_form_reads_no_pad_row(F0, triple):
    """A padded, already normalised batch (rows, T0, F0) with off[r] = r * T0 and no statistics: its pad rows hold NaN."""
    mats, cmvn, _, _ = case(F0)
    T0 = max(LENGTHS) + 2
    normed = [((m.astype(np.float64) - cmvn[0]) / cmvn[1]).astype(np.float32) for m in mats]
    batch = np.full((len(mats), T0, F0), np.nan, np.float32)
    for b, m in enumerate(normed):
        batch[b, : m.shape[0]] = m
    T_out = n_out(max(LENGTHS), triple[2])
    got = run(torch.from_numpy(batch).cuda(), [r * T0 for r in range(len(mats))], LENGTHS, triple, T_out, F0)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, expected(normed, triple, T_out))
    # ... which is the dataset's float64 normalisation followed by the splice (the float32 rounding commutes with copying rows)
    np.testing.assert_array_equal(got, expected(mats, triple, T_out, cmvn))


@pytest.mark.parametrize("triple", [(0, 2, 1), (2, 2, 3)], ids=lambda t: "%d-%d-%d" % t)
def test_t_out_clamps_the_output_rows(triple):
    """T_out smaller than the longest n_out (and no multiple of the chunk): rows past T_out do not exist, nothing behind the batch is
    written."""
    F0 = 80
    mats, cmvn, packed, offs = case(F0)
    T_out = n_out(33, triple[2]) - 1
    blocks = triple[0] + triple[1] + 1
    out = torch.full((len(LENGTHS) + 1, T_out, blocks * F0), -3.0, device="cuda")  # (one guard utterance behind the batch)
    hip.splice_rows(torch.from_numpy(packed).cuda(), i32(offs), i32(LENGTHS), out[: len(LENGTHS)], triple[0], triple[1], triple[2], PAD,
                    torch.from_numpy(cmvn[0]).cuda(), torch.from_numpy(cmvn[1]).cuda())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:-1], expected(mats, triple, T_out, cmvn))
    assert (got[-1] == -3.0).all()


@pytest.mark.parametrize("F0,triple", [(80, (0, 0, 8)), (80, (5, 5, 6)), (1000, (0, 2, 1)), (4, (64, 64, 64)), (83, (7, 0, 9))],
                         ids=["skip8", "wide", "F1000", "bounds", "odd"])
def test_spans_beyond_the_lds_shrink_the_chunk(F0, triple):
    """32 output frames of these shapes need more source rows than the kernel's LDS holds (or exactly the bounds: 64 / 64 / 64): the
    chunk shrinks, the values do not change.  skip > left + right + 1 also leaves span rows that no frame reads."""
    rng = np.random.default_rng(F0)
    lens = [200, 1, 131]
    mats = [rng.standard_normal((n, F0)).astype(np.float32) for n in lens]
    cmvn = (rng.standard_normal(F0) * 3 + 12, rng.random(F0) + 0.5)
    offs = [0, 200, 201]
    T_out = n_out(200, triple[2]) + 1
    got = run(torch.from_numpy(np.vstack(mats)).cuda(), offs, lens, triple, T_out, F0, cmvn)
    np.testing.assert_array_equal(got, expected(mats, triple, T_out, cmvn))


def test_a_source_off_the_16_byte_grid_takes_the_scalar_path():
    F0 = 80
    mats, cmvn, packed, offs = case(F0)
    flat = torch.full((packed.size + 1,), float("nan"), device="cuda")
    flat[1:] = torch.from_numpy(packed).cuda().reshape(-1)
    src = flat[1:]
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    got = run(src, offs, LENGTHS, (0, 2, 1), 66, F0, cmvn)
    np.testing.assert_array_equal(got, expected(mats, (0, 2, 1), 66, cmvn))


def test_negative_and_zero_lengths_give_padding():
    F0 = 80
    _, _, packed, offs = case(F0)
    got = run(torch.from_numpy(packed).cuda(), offs[:3], [0, -5, 31], (1, 1, 2), 20, F0)
    assert (got[:2] == PAD).all() and not (got[2, :16] == PAD).any() and (got[2, 16:] == PAD).all()


def test_refusals_leave_the_output_alone():
    L = hip.lib()
    F0 = 80
    _, _, packed, offs = case(F0)
    src, off, ln = torch.from_numpy(packed).cuda(), i32(offs), i32(LENGTHS)
    out = torch.full((7, 70, 3 * F0), 5.0, device="cuda")
    stat = torch.ones(F0, dtype=torch.float64, device="cuda")
    st, p = hip.current_stream(), hip._ptr

    def refused(src_=p(src), off_=p(off), len_=p(ln), out_=p(out), rows=7, T=70, F=F0, left=0, right=2, skip=1, mean=None, std=None):
        rc = L.cn_op_splice_rows(src_, off_, len_, out_, rows, T, F, left, right, skip, 0.0, mean, std, st)
        return rc != 0 and len(L.cn_last_error()) > 0

    assert refused(src_=None) and refused(off_=None) and refused(len_=None) and refused(out_=None)
    assert refused(mean=p(stat)) and refused(std=p(stat))  # one without the other
    assert refused(rows=0) and refused(T=0) and refused(F=0) and refused(rows=-1)
    assert refused(left=-1) and refused(right=-1) and refused(skip=-1)
    assert refused(rows=65536)
    assert refused(left=65) and refused(right=65) and refused(skip=65)  # the bounds: 64 / 64 / 64
    assert refused(F=5000)  # a spliced row of 15000 values: beyond the 12288 the LDS holds
    assert refused(rows=60000, T=60000, F=4)  # 4.3e10 values: beyond 32-bit indexing
    assert refused(rows=1, T=2 ** 30, F=1, left=0, right=0, skip=4)  # T_out * skip
    with pytest.raises(hip.HipError, match="64"):
        hip.splice_rows(src, off, ln, torch.empty(7, 70, 66 * F0, device="cuda"), 65, 0, 1, 0.0)
    torch.cuda.synchronize()
    assert (out == 5.0).all()
    assert not refused() and not refused(mean=p(stat), std=p(stat)) and not refused(skip=0)  # (and the same arguments are taken)
    torch.cuda.synchronize()
    assert not (out == 5.0).any()
