"""Every form of the integer kernels between the encoder and the decoder side against the exact models of tests/align_model.py
(which tests/test_align_model.py checks against the oracle and the reference's golden files first), through the C entry points.

Every comparison is exact (assert_array_equal; scores as equal float64 bits) and no tolerance appears anywhere: the alignment, pack,
plan, collapse, path, mask and record kernels do integer work, and the forced alignment's recursion is ONE float32 add of the same
two operands as the reference's (max over three predecessors + the frame's log-probability), with a strict `>` that keeps the first
maximum as torch.max does on the CPU - so alphas, back-pointers and path are bit-identical, ties among sums of -1e10 in unreachable
states included.  A case that disagrees is a finding to explain, not a reason for a margin.

Which test reaches which form bit and branch:
  test_ctc_align_plain          ctc_align_kernel, plain form: T' 1 / 2 (no scan carry, rows wider than the frames), 12, 255 / 256 /
                                257 (the 256-wide scan one short, full, one frame of a second chunk), 513 (a third chunk) x the four
                                (left, right) pairs; rows: full length, mask holes, no token, a token on the last valid frame, tokens
                                whose shifted frames are 255 / 256 / 257 (carry across the chunk boundary), src_size 0 (EOS frame wraps
                                to T' - 1), src_size one short of the mask, a masked frame with a non-blank label (zeroed)
  test_ctc_align_forms          raw_path + ylen_in (masked labels kept, given counts), src_mod (G = 3), utt_meta (T' {Tp, Tp - 3, 1}:
                                shift 0 at and past T' - a token that starts on its batch's last frame is dropped -, src_size from
                                T', poisoned labels behind T', an utterance without a valid frame), no_trigger (rows = the whole
                                range, no EOS row in ylen / ymax), no_trigger + utt_meta, src_mod + utt_meta, raw_path + utt_meta;
                                T' 12 and 257 each.  The frame a src_size of 0 wraps to: the EOS row of the path's OWN count always
                                holds the last frame already (c[T' - 1] is that count), so the wrap shows only where ylen_in names
                                a count the path does not reach - row 5 of the raw_path forms, wrapping to T' - 1 and, under
                                utt_meta, to the batch's own T' - 1
  test_ctc_align_refusals       a T' whose rows exceed 160 KiB of LDS: error, nothing written; null pointer; a record's T' > Tp
  test_ctc_viterbi              ctc_viterbi_kernel: (6, 40, 12, 9), (3, 300, 12, 130) (2 ymax + 1 = 261 states: the per-state loops'
                                second trip), (4, 1, 5, 1); zero labels (plen - 2 wraps to state S - 1), all labels equal, more labels
                                than frames fit, label_len < ymax with garbage behind the count, mask holes, xb 0 / 1 / Tp, ld > ymax;
                                out_path itself, then the chain through cn_op_ctc_align_desc (raw_path + ylen_in) against
                                oracle.viterbi_align + align_to_intervals
  test_ctc_viterbi_refusal      ymax = 0
  test_greedy_pack_and_plan     greedy_pack_kernel / row_plan_kernel on the same limits: sub = 4 with B = 11, utt_meta of three uneven
                                batches, *ymax_dev = 6 < U, hyp_stride = 5, row_off from cn_op_row_plan, all of them together
  test_row_plan_second_chunk    B = 300: the plan's scan carry, and the pack kernel on its offsets
  test_no_trigger_silent_batch  ylen all 0: zero rows in both kernels
  test_greedy_pack_refusals     cn_op_greedy_pack_rows reads utt_meta and row_off back: a batch outside 0 .. B, offsets beyond b * U or
                                decreasing, null, B < 1 (cn_op_greedy_pack too) - nothing written
  test_ctc_collapse             ctc_collapse_kernel: T' 1 / 63 / 64 / 65 / 130 (the wave's 64-frame trips); all blank, one label,
                                alternating labels (T' tokens), masked frames between equal labels, ld = T' + 1 and ld > T' + 1
  test_ctc_collapse_refusal     ld = T', with a message
  test_esa_paths                esa_paths_kernel: M = 300 (two blocks), n = 1 with null select and n = 3; exp(v) == threshold exactly
  test_keymask                  keymask_kernel: 4 (T' - 1) below T (and equal to T - 1, the last frame), EQUAL to T (the first frame
                                that does not exist: masked for every utterance) and beyond T, guard frames behind the buffer; the
                                padding value in column 0 only / in the other columns only; F = 3
  test_expand_meta              expand_meta_kernel: n = 1, n = 64, B beyond the rows' sum, frames 1 / 2 / 5 / 64; refusals n = 0 / 65

Departures from the reference semantics found while the models were written, fixed in the kernels and held by these tests:
  * ctc_viterbi_kernel left the whole path blank for src_size 0, where the reference's `aligned[b, xb - 1]` wraps to the LAST frame and
    puts the final state's label there (test_ctc_viterbi, xb = 0 rows).  Only the path differed: the shift the decoder reads is one
    frame late and never holds the last frame's label, so no decode changed.
  * launch_ctc_align zeroed *ymax before it refused a T' beyond its LDS (test_ctc_align_refusals: nothing is written);
    launch_ctc_collapse refused without a message (test_ctc_collapse_refusal).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import align_cases as ac
import align_model as am
from cassnat_asr_public_amd import hip
from oracle import cassnat_oracle as orc

pytestmark = pytest.mark.gpu
POISON = -77


def dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).contiguous().cuda()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ip(t):
    return None if t is None else t.data_ptr()


def out_i32(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda")


def last_error():
    return hip.lib().cn_last_error().decode(errors="replace")


# ------------------------------------------------------------------------------------------------------------ ctc_align
def run_align(best, mask, ratio, left=0, right=0, raw_path=False, ylen_in=None, src_mod=0, utt_meta=None, no_trigger=False, plain_entry=False):
    """-> (shift, src_size, ylen, ymax, intervals (B, Tp + 1, 4)) as numpy arrays."""
    B, Tp = best.shape
    shift, src, ylen, ymax, iv = out_i32(B, Tp), out_i32(B), out_i32(B), out_i32(1), out_i32(B, Tp + 1, 4)
    bd, md, rd = dev(best, torch.int32), dev(mask, torch.uint8), dev(ratio, torch.float32)
    yd = None if ylen_in is None else dev(ylen_in, torch.int32)
    ud = None if utt_meta is None else dev(utt_meta, torch.int32)
    L = hip.lib()
    if plain_entry:
        hip.check(L.cn_op_ctc_align(p(bd), p(md), p(rd), B, Tp, 0, left, right, p(shift), p(src), p(ylen), p(ymax), p(iv), hip.current_stream()),
                  "cn_op_ctc_align")
    else:
        d = hip.CnAlignDesc(best=ip(bd), keymask=ip(md), size_ratio=ip(rd), B=B, Tp=Tp, blank=0, left=left, right=right, src_mod=src_mod,
                            shift=ip(shift), src_size=ip(src), ylen=ip(ylen), ymax=ip(ymax), intervals=ip(iv), raw_path=int(raw_path),
                            ylen_in=ip(yd), utt_meta=ip(ud), no_trigger=int(no_trigger))
        hip.check(L.cn_op_ctc_align_desc(C.byref(d), hip.current_stream()), "cn_op_ctc_align_desc")
    torch.cuda.synchronize()
    return shift.cpu().numpy(), src.cpu().numpy(), ylen.cpu().numpy(), int(ymax.item()), iv.cpu().numpy()


def dense_from_intervals(iv, mask, rows):
    """The dense trigger rows the attention kernel sees: the two intervals of a row, ANDed with the key mask."""
    t = np.arange(mask.shape[1])[None, None, :]
    s1, e1, s2, e2 = (iv[:, :rows, i][:, :, None] for i in range(4))
    return (((t >= s1) & (t < e1)) | ((t >= s2) & (t < e2))) & mask[:, None, :]


def check_align(got, want, mask, tp, no_trigger=False):
    """got: run_align's tuple; want: align_model's; mask (B, Tp) per entry; tp (B,) each entry's own width."""
    shift, src, ylen, ymax, iv = got
    w_shift, w_src, w_ylen, w_ymax, w_trig = want
    B, Tp = shift.shape
    np.testing.assert_array_equal(shift, w_shift)
    np.testing.assert_array_equal(src, w_src)
    np.testing.assert_array_equal(ylen, w_ylen)
    assert ymax == w_ymax
    np.testing.assert_array_equal(dense_from_intervals(iv, mask, ymax), w_trig)
    assert (iv != POISON).all() and (iv >= 0).all() and (iv[:, :, 1::2] <= tp[:, None, None]).all()  # every row written, inside the own width
    for b in range(B):
        assert not shift[b, tp[b]:].any()  # no token is carried onto a frame the utterance's own batch does not have
        if no_trigger:  # every row, used or not, is the whole range
            np.testing.assert_array_equal(iv[b], np.tile([0, tp[b], 0, 0], (Tp + 1, 1)))
        else:  # rows past the EOS row are empty
            assert not (iv[b, ylen[b]:, 1] > iv[b, ylen[b]:, 0]).any() and not (iv[b, ylen[b]:, 3] > iv[b, ylen[b]:, 2]).any()
            assert not (iv[b, :ylen[b] - 1, 3] > iv[b, :ylen[b] - 1, 2]).any()  # the second interval belongs to the EOS row alone


@pytest.mark.parametrize("left,right", ac.TRIGGERS)
@pytest.mark.parametrize("Tp", ac.ALIGN_TP)
def test_ctc_align_plain(Tp, left, right):
    best, mask, ratio, _ = ac.align_case(Tp)
    want = am.align_model(best, mask, ratio, left, right)
    tp = np.full(best.shape[0], Tp)
    check_align(run_align(best, mask, ratio, left, right), want, mask, tp)
    if (left, right) == (1, 0):  # cn_op_ctc_align is the same code
        check_align(run_align(best, mask, ratio, left, right, plain_entry=True), want, mask, tp)


@pytest.mark.parametrize("form", ac.ALIGN_FORMS)
@pytest.mark.parametrize("Tp", [12, 257])
def test_ctc_align_forms(Tp, form):
    kw = ac.align_form_case(Tp, form)
    want = am.align_model(**kw)
    B, Bs = kw["best"].shape[0], kw["mask"].shape[0]
    rows = np.arange(B) % Bs
    tp = kw["utt_meta"][rows, 1] if "utt_meta" in kw else np.full(B, Tp)
    check_align(run_align(**kw), want, kw["mask"][rows], tp, kw.get("no_trigger", False))


def test_ctc_align_refusals():
    """The refusals return before anything is launched or written."""
    L = hip.lib()
    Tp = 20350  # (256 + 4 + 2 (Tp + 1)) ints = 163848 bytes > 160 KiB; 20349 frames fit exactly
    shift, src, ylen, ymax, iv = out_i32(1, Tp), out_i32(1), out_i32(1), out_i32(1), out_i32(1, Tp + 1, 4)
    bd, md, rd = dev(np.ones((1, Tp)), torch.int32), dev(np.ones((1, Tp)), torch.uint8), dev([1.0], torch.float32)
    f = dict(best=ip(bd), keymask=ip(md), size_ratio=ip(rd), B=1, Tp=Tp, shift=ip(shift), src_size=ip(src), ylen=ip(ylen), ymax=ip(ymax),
             intervals=ip(iv))
    assert L.cn_op_ctc_align_desc(C.byref(hip.CnAlignDesc(**f)), hip.current_stream()) == -1 and "LDS" in last_error()
    torch.cuda.synchronize()
    for t in (shift, src, ylen, ymax, iv):
        assert (t == POISON).all()
    assert L.cn_op_ctc_align_desc(C.byref(hip.CnAlignDesc(**dict(f, Tp=12, ymax=None))), hip.current_stream()) == -1 and "null" in last_error()
    assert L.cn_op_ctc_align_desc(C.byref(hip.CnAlignDesc(**dict(f, Tp=12, B=0))), hip.current_stream()) == -1
    assert L.cn_op_ctc_align_desc(None, hip.current_stream()) == -1
    ud = dev([[49, 13, 0, 1]], torch.int32)  # a record wider than the call
    assert L.cn_op_ctc_align_desc(C.byref(hip.CnAlignDesc(**dict(f, Tp=12, utt_meta=ip(ud)))), hip.current_stream()) == -1 and "utt_meta" in last_error()
    torch.cuda.synchronize()
    assert (ymax == POISON).all() and (shift == POISON).all()
    assert L.cn_align_desc_size() == C.sizeof(hip.CnAlignDesc)


# ------------------------------------------------------------------------------------------------------------ ctc_viterbi
def run_viterbi(c, ymax):
    B, Tp, V = c["logp"].shape
    out = out_i32(B, Tp)
    ld = c["labels"].shape[1]
    args = [dev(c["logp"], torch.float32), dev(c["mask"], torch.uint8), dev(c["ratio"], torch.float32), dev(c["labels"], torch.int32),
            dev(c["ylens"], torch.int32)]
    rc = hip.lib().cn_op_ctc_viterbi(*[p(a) for a in args], B, Tp, V, ld, ymax, 0, p(out), hip.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("shape", ac.VITERBI_SHAPES)
def test_ctc_viterbi(shape):
    B, Tp, V, ymax = shape
    c = ac.viterbi_case(*shape)
    labels, shift = am.viterbi_model(c["logp"], c["mask"], c["ratio"], c["ys"], c["ylens"])
    rc, path = run_viterbi(c, ymax)
    hip.check(rc, "cn_op_ctc_viterbi")
    np.testing.assert_array_equal(path, labels)
    # the chain the engine runs: the path through the alignment kernel's forced form
    src = orc.src_size_frames(c["ratio"], Tp)
    for left, right in ((0, 0), (1, 1)):
        o_trig, o_ylen, o_ymax = orc.align_to_intervals(shift, c["ylens"], int(c["ylens"].max()), c["mask"], src, 0, left, right)
        got = run_align(path, c["mask"], c["ratio"], left, right, raw_path=True, ylen_in=c["ylens"])
        check_align(got, (shift, src, o_ylen, o_ymax, o_trig), c["mask"], np.full(B, Tp))


def test_ctc_viterbi_refusal():
    c = ac.viterbi_case(*ac.VITERBI_SHAPES[2])
    rc, path = run_viterbi(c, 0)
    assert rc == -1 and "ymax" in last_error() and (path == POISON).all()


# ------------------------------------------------------------------------------------------------------------ greedy pack / row plan
def run_plan(ylen, U, hyp_stride, sub, utt_meta, ymax):
    B = len(ylen)
    yd, md = dev(ylen, torch.int32), None if utt_meta is None else dev(utt_meta, torch.int32)
    xd = None if ymax is None else dev([ymax], torch.int32)
    off = out_i32(B + 1)
    hip.check(hip.lib().cn_op_row_plan(p(yd), B, U, hyp_stride, sub, p(md), p(xd), p(off), hip.current_stream()), "cn_op_row_plan")
    torch.cuda.synchronize()
    return off


def run_pack(tok, val, ylen, U, hyp_stride, sub, utt_meta, ymax, row_off):
    """tok / val: flat device-shaped arrays (padded (B, U) or packed); row_off: a device tensor or None."""
    B = len(ylen)
    hyp, hl = out_i32(B, hyp_stride), out_i32(B)
    sc = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    td, vd, yd = dev(tok, torch.int32), dev(val, torch.float32), dev(ylen, torch.int32)
    md = None if utt_meta is None else dev(utt_meta, torch.int32)
    xd = None if ymax is None else dev([ymax], torch.int32)
    hip.check(hip.lib().cn_op_greedy_pack_rows(p(td), p(vd), p(yd), B, U, 1, hyp_stride, p(hyp), p(hl), p(sc), sub, p(md), p(xd), p(row_off),
                                               hip.current_stream()), "cn_op_greedy_pack_rows")
    torch.cuda.synchronize()
    return hyp.cpu().numpy(), hl.cpu().numpy(), sc.cpu().numpy()


def check_pack_and_plan(ylen, kw, tok, val):
    """Both kernels on the same limit arguments: the plan against row_count_model, the pack against greedy_pack_model, and each other."""
    B, U, stride = len(ylen), kw["U"], kw["hyp_stride"]
    lim = dict(sub=kw["sub"], utt_meta=kw["utt_meta"], ymax=kw["ymax"])
    off = run_plan(ylen, U, stride, **lim)
    w_off = am.row_off_model(ylen, U, stride, **lim)
    np.testing.assert_array_equal(off.cpu().numpy(), w_off)
    rows = np.diff(w_off)
    if kw["packed"]:  # the rows nobody owns are poisoned: a read past an utterance's count shows
        tok_in = np.concatenate([tok[b, :rows[b]] for b in range(B)] + [np.full(B * U - w_off[-1], POISON)])
        val_in = np.concatenate([val[b, :rows[b]] for b in range(B)] + [np.full(B * U - w_off[-1], np.nan, np.float32)])
    else:
        tok_in, val_in = tok.reshape(-1), val.reshape(-1)
    hyp, hl, sc = run_pack(tok_in, val_in, ylen, U, stride, row_off=off if kw["packed"] else None, **lim)
    w_hyp, w_hl, w_sc = am.greedy_pack_model(tok_in, val_in, ylen, U, 1, stride, row_off=w_off if kw["packed"] else None, **lim)
    np.testing.assert_array_equal(hyp, w_hyp)
    np.testing.assert_array_equal(hl, w_hl)
    np.testing.assert_array_equal(sc.view(np.int64), w_sc.view(np.int64))  # the sequential double sum, bit for bit
    np.testing.assert_array_equal(np.diff(off.cpu().numpy()), hl - 1)  # "the SAME limit rule": the plan's rows are the pack's
    return rows


@pytest.mark.parametrize("kind", ac.PACK_CASES)
def test_greedy_pack_and_plan(kind):
    ylen, kw = ac.pack_case(kind)
    tok, val = ac.pack_rows(len(ylen), kw["U"])
    rows = check_pack_and_plan(ylen, kw, tok, val)
    # the limit each case is about binds somewhere
    if kind == "sub":  # (utterance 0 holds U rows; the last batch, of three, is limited by its own largest ylen)
        assert rows[0] == kw["U"] and rows[8:].max() == ylen[8:].max() < kw["U"]
    if kind == "utt_meta":
        assert rows[5] == 1 and rows[6:].max() == ylen[6:].max() <= 4
    if kind in ("ymax_dev", "hyp_stride", "all"):
        assert rows.max() == {"ymax_dev": 6, "hyp_stride": 4, "all": 4}[kind]


def test_row_plan_second_chunk():
    """B = 300: the plan's scan runs a second 256-wide chunk and carries the first one's total."""
    rng = np.random.default_rng(6)
    B, U = 300, 9
    ylen = rng.integers(1, U + 1, size=B)
    tok, val = ac.pack_rows(B, U, seed=1)
    rows = check_pack_and_plan(ylen, dict(U=U, hyp_stride=U + 2, sub=7, utt_meta=None, ymax=8, packed=True), tok, val)
    assert rows[:256].sum() > 0 and rows[256:].sum() > 0


def test_no_trigger_silent_batch():
    """use_trigger off: ylen carries no EOS row, and a batch in which nobody has a token has no decoder row at all - in both kernels."""
    B, U = 11, 9
    ylen = np.zeros(B, np.int64)
    tok, val = ac.pack_rows(B, U)
    for lim in (dict(sub=0, utt_meta=None, ymax=0), dict(sub=4, utt_meta=None, ymax=None), dict(sub=0, utt_meta=ac.meta_of([5, 1, 5], [7, 7, 7]), ymax=None)):
        for packed in (False, True):
            rows = check_pack_and_plan(ylen, dict(U=U, hyp_stride=U + 2, packed=packed, **lim), tok, val)
            assert not rows.any()
    # one batch with tokens beside two silent ones: only its utterances get rows
    ylen[5] = 3
    rows = check_pack_and_plan(ylen, dict(U=U, hyp_stride=U + 2, packed=True, sub=0, utt_meta=ac.meta_of([5, 1, 5], [7, 7, 7]), ymax=3), tok, val)
    assert rows.tolist() == [0] * 5 + [3] + [0] * 5


def test_greedy_pack_refusals():
    """The device records the kernel indexes by are read back: a batch outside the call, offsets past the rows tok / val hold, offsets
    that decrease - refused with nothing written, as are a null pointer and B < 1 (the older entry, the same code, included)."""
    B, U = 4, 5
    tok, val = ac.pack_rows(B, U)
    td, vd, yd = dev(tok, torch.int32), dev(val, torch.float32), dev([3, 5, 1, 2], torch.int32)
    hyp, hl = out_i32(B, U + 2), out_i32(B)
    sc = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    L = hip.lib()

    def call(meta=None, off=None, B_=B, tokp=td):
        md, od = (None if a is None else dev(a, torch.int32) for a in (meta, off))
        rc = L.cn_op_greedy_pack_rows(p(tokp), p(vd), p(yd), B_, U, 1, U + 2, p(hyp), p(hl), p(sc), 0, p(md), None, p(od), hip.current_stream())
        torch.cuda.synchronize()
        return rc

    for kw, why in ((dict(meta=[[0, 0, 0, 2]] * 2 + [[0, 0, 2, 5]] * 2), "utt_meta"), (dict(meta=[[0, 0, -1, 2]] * 4), "utt_meta"),
                    (dict(meta=[[0, 0, 3, 2]] * 4), "utt_meta"), (dict(off=[0, 6, 7, 8, 9]), "row_off"), (dict(off=[0, 4, 3, 8, 9]), "row_off"),
                    (dict(off=[-1, 4, 6, 8, 9]), "row_off"), (dict(off=[0, 4, 6, 8, 21]), "row_off"), (dict(B_=0), "B, U"), (dict(tokp=None), "null")):
        assert call(**kw) == -1 and why in last_error(), kw
        assert (hyp == POISON).all() and (hl == POISON).all() and torch.isnan(sc).all()
    assert L.cn_op_greedy_pack(p(td), p(vd), p(yd), 0, U, 1, U + 2, p(hyp), p(hl), p(sc), hip.current_stream()) == -1 and "cn_op_greedy_pack:" in last_error()
    assert call(meta=[[0, 0, 0, 2]] * 2 + [[0, 0, 2, 4]] * 2, off=[0, 4, 9, 11, 13]) == 0 and hl.cpu().tolist() == [5, 6, 3, 3]


# ------------------------------------------------------------------------------------------------------------ ctc_collapse
def run_collapse(best, mask, sos, pad, ld):
    B, Tp = best.shape
    tgt, n, keylen, maxlen = out_i32(B, ld), out_i32(B), out_i32(B), out_i32(1)
    bd, md = dev(best, torch.int32), dev(mask, torch.uint8)
    rc = hip.lib().cn_op_ctc_collapse(p(bd), p(md), B, Tp, sos, pad, ld, p(tgt), p(n), p(keylen), p(maxlen), hip.current_stream())
    torch.cuda.synchronize()
    return rc, tgt.cpu().numpy(), n.cpu().numpy(), keylen.cpu().numpy(), maxlen.cpu().numpy()


@pytest.mark.parametrize("extra", [1, 4])
@pytest.mark.parametrize("Tp", ac.COLLAPSE_TP)
def test_ctc_collapse(Tp, extra):
    best, mask = ac.collapse_case(Tp)
    rc, tgt, n, keylen, maxlen = run_collapse(best, mask, 1, 9, Tp + extra)
    hip.check(rc, "cn_op_ctc_collapse")
    w_tgt, w_n, w_keylen, w_maxlen = am.collapse_model(best, mask, 1, 9, Tp + extra)
    np.testing.assert_array_equal(tgt, w_tgt)
    np.testing.assert_array_equal(n, w_n)
    np.testing.assert_array_equal(keylen, w_keylen)
    assert maxlen.tolist() == [w_maxlen] and w_maxlen == Tp


def test_ctc_collapse_refusal():
    best, mask = ac.collapse_case(12)
    rc, tgt, n, _, maxlen = run_collapse(best, mask, 1, 9, 12)
    assert rc == -1 and "ld" in last_error() and (tgt == POISON).all() and (n == POISON).all() and (maxlen == POISON).all()
    assert hip.lib().cn_op_ctc_collapse(None, None, 1, 1, 1, 0, 2, None, None, None, None, hip.current_stream()) == -1 and "null" in last_error()


# ------------------------------------------------------------------------------------------------------------ esa_paths
@pytest.mark.parametrize("n", [1, 3])
def test_esa_paths(n):
    rng = np.random.default_rng(70 + n)
    M = 300
    idx = np.stack([rng.permutation(40)[:2] for _ in range(M)])
    for threshold, values in ((0.5, (0.2, 0.8)), (1.0, (0.2, 1.0))):  # exp(log 1) == 1 exactly: not below the threshold
        val = np.log(np.array(values, np.float32))[rng.integers(0, 2, size=M)]
        val = np.stack([val, val - 1], 1).astype(np.float32)
        select = None if n == 1 else rng.integers(0, 2, size=(n, M)).astype(np.uint8)
        want = am.esa_paths_model(idx, val, select, threshold)
        assert select is None or ((want != idx[None, :, 0]).any() and (want[:, val[:, 0] == 0] == idx[val[:, 0] == 0, 0]).all())
        best = out_i32(n, M)
        idd, vd, sd = dev(idx, torch.int32), dev(val, torch.float32), None if select is None else dev(select, torch.uint8)
        hip.check(hip.lib().cn_op_esa_paths(p(idd), p(vd), p(sd), threshold, p(best), M, n, hip.current_stream()), "cn_op_esa_paths")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(best.cpu().numpy(), want)
    assert hip.lib().cn_op_esa_paths(p(idd), p(vd), None, 0.5, p(best), 0, 1, hip.current_stream()) == -1 and "M and n" in last_error()


# ------------------------------------------------------------------------------------------------------------ keymask
@pytest.mark.parametrize("T,Tp", [(30, 7), (25, 7), (24, 7), (23, 7), (4, 2), (9, 4), (1, 1)])
def test_keymask(T, Tp):
    """The last subsampled frame reads input frame 4 (Tp - 1) = 24: below T (30; 25, where it is the batch's last frame), EQUAL to T
    (24: the first frame that does not exist - masked for every utterance, the full-length utterance 0 included) and beyond T (23).
    (4, 2) the same equality at the smallest size, (9, 4) a frame three past the batch.  The frames behind an utterance are the next
    utterance's valid first frames, and the device buffer ends in four guard frames of ones, so a kernel that read frame T or T + 1
    would stay inside the buffer and call them valid."""
    rng = np.random.default_rng(T)
    B, F = 5, 3
    feats = rng.standard_normal((B, T, F)).astype(np.float32)
    lens = rng.integers(1, T + 1, size=B)
    lens[0] = lens[B - 1] = T
    feats[np.arange(T)[None, :] >= lens[:, None]] = 0
    j = (Tp - 1) // 2
    feats[1, 4 * j, 0] = 0    # the padding value in column 0 only: masked
    feats[2, 4 * j, 1:] = 0   # in the other columns only: valid
    want = am.keymask_model(feats, Tp)
    assert not want[1, j] and (want[2, j] or 4 * j >= lens[2]) and (feats[[0, 2, 3, 4], 0, 0] != 0).all()
    if 4 * (Tp - 1) >= T:
        assert not want[:, Tp - 1].any()
    elif 4 * (Tp - 1) == T - 1:
        assert want[0, Tp - 1] and want[B - 1, Tp - 1]
    km = torch.full((B, Tp), 7, dtype=torch.uint8, device="cuda")
    fd = dev(np.concatenate([feats.reshape(-1), np.ones(4 * F, np.float32)]), torch.float32)
    hip.check(hip.lib().cn_op_keymask(p(fd), B, T, F, Tp, 4, 0.0, p(km), hip.current_stream()), "cn_op_keymask")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(km.cpu().numpy(), want.astype(np.uint8))
    assert hip.lib().cn_op_keymask(p(fd), B, T, F, Tp, 0, 0.0, p(km), hip.current_stream()) == -1 and "stride" in last_error()


# ------------------------------------------------------------------------------------------------------------ expand_meta
def run_expand(rows, frames, B, n=None):
    meta = out_i32(B, 4)
    r, f = (C.c_int32 * len(rows))(*rows), (C.c_int32 * len(frames))(*frames)
    rc = hip.lib().cn_op_expand_meta(r, f, len(rows) if n is None else n, p(meta), B, hip.current_stream())
    torch.cuda.synchronize()
    return rc, meta.cpu().numpy()


@pytest.mark.parametrize("rows,frames,B", [
    ([5], [64], 5),                                              # one batch
    ([1, 2, 3, 4], [1, 2, 5, 64], 10),                           # the two (x - 1) / 2 + 1 steps: T' 1, 1, 2, 16
    ([2, 3], [9, 33], 9),                                        # B beyond the rows' sum: the last batch's record for the rest
    (list(range(1, 65)), [1 + 3 * k for k in range(64)], 2080),  # the largest list; more than one block of utterances
])
def test_expand_meta(rows, frames, B):
    rc, meta = run_expand(rows, frames, B)
    hip.check(rc, "cn_op_expand_meta")
    np.testing.assert_array_equal(meta, am.expand_meta_model(rows, frames, B))


def test_expand_meta_refusals():
    """An empty list, one batch more than CN_MAX_SUB = 64, a batch without rows: refused before the launch."""
    for rows, n, why in (([1], 0, "1 .. 64"), ([1] * 65, None, "1 .. 64"), ([1, 0], None, "rows >= 1")):
        rc, meta = run_expand(rows, [8] * len(rows), 4, n)
        assert rc == -1 and why in last_error() and (meta == POISON).all()
