"""Plain numpy models of the integer kernels between the encoder and the decoder side (ctc_align.hip, ctc_beam.hip's forced
alignment, rowops.hip's path / mask / record kernels), one function per kernel: int64 / float32 / float64, none of this
project's kernels.  Each is written from the reference semantics the kernels' comments quote (src/models/cassnat.py:259-270,
272-353, 355-389, 436, 468-473, 574-637; src/models/transformer.py:256-270; src/tasks/cassnat_task.py:328), not from the kernels'
code; the alignment itself is oracle.cassnat_oracle's.  tests/test_align_model.py checks them against the golden files and the
oracle before tests/test_gpu_align_kernels.py lets them judge a kernel."""
import numpy as np

from oracle import cassnat_oracle as orc

LOGZERO = np.float32(-1e10)


def subsampled(frames):
    """T' of `frames` frames behind the two stride-2 convolutions (embedding.py:102-108)."""
    return ((frames - 1) // 2 + 1 - 1) // 2 + 1


def collapse_shift(labels, blank=0):
    """Per-frame labels -> aligned_seq_shift (cassnat.py:346-352, 385-388): repeats of the previous frame zeroed, one frame later."""
    labels = np.asarray(labels, np.int64)
    prev = np.zeros_like(labels)
    prev[:, 1:] = labels[:, :-1]
    collapsed = np.where(labels == prev, 0, labels)
    shift = np.zeros_like(labels)
    shift[:, 1:] = collapsed[:, :-1]
    return shift


def _align_one(best, mask, ratio, left, right, raw_path, ylen_in, no_trigger, blank):
    """One reference batch at its own width: (shift, src_size, ylen, trigger rows as a dense bool array)."""
    B, Tp = best.shape
    src = orc.src_size_frames(ratio, Tp)
    if raw_path:  # a forced alignment's labels are collapsed as they are (viterbi_align does not mask them)
        shift = collapse_shift(best, blank)
        ylen0 = (shift != blank).sum(1)
    else:
        shift, ylen0, _ = orc.best_path_align(best, mask, blank)
    if ylen_in is not None:  # viterbi_align hands its input label counts on
        ylen0 = np.asarray(ylen_in, np.int64)
    ymax0 = int(ylen0.max())
    if no_trigger:  # trigger_mask = src_mask (cassnat.py:469-473): align_to_mask does not run, no EOS row is added
        return shift, src, ylen0, np.zeros((B, 0, Tp), bool)  # (align_model fills the rows in)
    trig, ylen, _ = orc.align_to_intervals(shift, ylen0, ymax0, mask, src, blank, left, right)
    return shift, src, ylen, trig


def align_model(best, mask, ratio, left=0, right=0, raw_path=False, ylen_in=None, src_mod=0, utt_meta=None, no_trigger=False, blank=0):
    """ctc_align_kernel.  best (B, Tp) int; mask (Bs, Tp) bool, ratio (Bs,) float32 and utt_meta (Bs, 4) int (frames, T', first, one
    past the last; None: one batch of width Tp) with Bs = src_mod if src_mod > 0 else B - entry b reads row b % src_mod of them.
    Returns (shift (B, Tp) int64, src_size (B,), ylen (B,), ymax, trigger (B, ymax, Tp) bool): every reference batch is aligned
    alone at its own width and padded (zeros / False) to the call's; ymax is the call's largest ylen."""
    best, mask = np.asarray(best, np.int64), np.asarray(mask, bool)
    ratio = np.asarray(ratio, np.float32)
    B, Tp = best.shape
    if src_mod > 0:  # the ESA draws of an utterance share its mask, its ratio and its batch
        rows = np.arange(B) % src_mod
        mask, ratio = mask[rows], ratio[rows]
        utt_meta = None if utt_meta is None else np.asarray(utt_meta)[rows]
    ylen_in = None if ylen_in is None else np.asarray(ylen_in, np.int64)
    if utt_meta is None:
        groups = [(Tp, np.arange(B))]
    else:
        utt_meta = np.asarray(utt_meta, np.int64)
        keys = sorted({(int(m[2]), int(m[3]), int(m[1])) for m in utt_meta})
        groups = [(tp, np.nonzero((utt_meta[:, 2] == lo) & (utt_meta[:, 3] == hi))[0]) for lo, hi, tp in keys]
    shift = np.zeros((B, Tp), np.int64)
    src, ylen, trigs = np.zeros(B, np.int64), np.zeros(B, np.int64), {}
    for tp, rows in groups:
        s, z, y, t = _align_one(best[rows, :tp], mask[rows, :tp], ratio[rows], left, right, raw_path,
                                None if ylen_in is None else ylen_in[rows], no_trigger, blank)
        shift[rows, :tp], src[rows], ylen[rows] = s, z, y
        trigs[tp] = (rows, t)
    ymax = int(ylen.max())
    trig = np.zeros((B, ymax, Tp), bool)
    for tp, (rows, t) in trigs.items():
        trig[rows[:, None, None], np.arange(t.shape[1])[None, :, None], np.arange(tp)[None, None, :]] = t
    if no_trigger:  # every row is the utterance's mask over the frames its own batch has, whatever that batch's own ymax
        own = np.arange(Tp)[None, :] < (Tp if utt_meta is None else utt_meta[:, 1:2])
        trig[:] = (mask & own)[:, None, :]
    return shift, src, ylen, ymax, trig


def viterbi_model(logp, mask, ratio, ys, ylens, blank=0):
    """ctc_viterbi_kernel: CassNAT.viterbi_align (cassnat.py:272-353, sample_topk 0).  logp (B, Tp, V) float32, mask (B, Tp) bool,
    ratio (B,) float32, ys (B, ymax) int zero padded, ylens (B,).  Returns (labels (B, Tp) int64: the label of the aligned state per
    frame - `torch.gather(path, 1, aligned)`, before the collapse -, shift (B, Tp) int64 = oracle.viterbi_align's result).  The
    recursion is restated here in float32 (the oracle does not return its path) and its collapsed shift must be the oracle's."""
    logp, mask = np.asarray(logp, np.float32), np.asarray(mask, bool)
    ys, ylens = np.asarray(ys, np.int64), np.asarray(ylens, np.int64)
    B, Tp, _ = logp.shape
    ymax = ys.shape[1]
    L = 2 * ymax + 1
    src = orc.src_size_frames(ratio, Tp)
    path = np.full((B, L), blank, np.int64)
    path[:, 1::2] = ys
    plen = 2 * ylens + 1
    lp = np.where(mask[:, :, None], logp, LOGZERO)
    lp_path = np.take_along_axis(lp, np.repeat(path[:, None, :], Tp, 1), 2)  # (B, Tp, L)
    alpha = np.full((Tp + 1, B, L), LOGZERO, np.float32)
    alpha[0, :, 0] = 0
    same = path[:, :-2] == path[:, 2:]
    outside = np.arange(L)[None, :] >= plen[:, None]
    bp = np.zeros((B, Tp, L), np.int64)
    for t in range(Tp):
        mat = np.full((3, B, L), LOGZERO, np.float32)
        mat[0] = alpha[t]
        mat[1, :, 1:] = alpha[t, :, :-1]
        mat[2, :, 2:] = np.where(same, LOGZERO, alpha[t, :, :-2])
        idx = mat.argmax(0)  # the first maximum, as torch.max on the CPU
        mx = np.take_along_axis(mat, idx[None], 0)[0]
        mx[outside] = LOGZERO
        bp[:, t, :] = np.arange(L)[None, :] - idx
        alpha[t + 1] = mx + lp_path[:, t, :]
    aligned = np.zeros((B, Tp), np.int64)
    for b in range(B):
        xb, yb = int(src[b]), int(plen[b])
        aligned[b, xb - 1] = yb - 1 if alpha[xb, b, yb - 1] > alpha[xb, b, yb - 2] else yb - 2  # (negative indices wrap, as in torch)
        for t in range(xb - 1, 0, -1):
            aligned[b, t - 1] = bp[b, t, aligned[b, t]]
    labels = np.take_along_axis(path, aligned, 1)
    shift = orc.viterbi_align(logp, mask, src, ys, ylens, blank)
    np.testing.assert_array_equal(collapse_shift(labels, blank), shift, err_msg="viterbi_model's path does not collapse to the oracle's shift")
    return labels, shift


def collapse_model(best, mask, sos, pad, ld):
    """ctc_collapse_kernel: Transformer.fast_decode_with_ctc's decoder input (transformer.py:256-270).  Returns (tgt (B, ld) int64,
    len (B,), keylen (B,), maxlen)."""
    best, mask = np.asarray(best, np.int64), np.asarray(mask, bool)
    B, Tp = best.shape
    assert ld >= Tp + 1
    path = np.where(mask, best, 0)
    prev = np.zeros_like(path)
    prev[:, 1:] = path[:, :-1]
    collapsed = np.where(path == prev, 0, path)
    tgt = np.full((B, ld), pad, np.int64)
    tgt[:, 0] = sos
    n = np.zeros(B, np.int64)
    for b in range(B):
        lab = collapsed[b][collapsed[b] != 0]
        n[b] = lab.size
        tgt[b, 1:1 + lab.size] = lab
    return tgt, n, n + 1, int(n.max())


def esa_paths_model(top2_idx, top2_val, select, threshold):
    """esa_paths_kernel (cassnat.py:370-376): top2_idx / top2_val (M, 2), select (n, M) 0 / 1 draws or None (one path: the best).
    Frame i of path g takes the second best label iff its draw is 1 and exp(best log-prob) < threshold, in float32, strictly."""
    top2_idx, top2_val = np.asarray(top2_idx, np.int64), np.asarray(top2_val, np.float32)
    if select is None:
        return top2_idx[None, :, 0].copy()
    low = np.exp(top2_val[:, 0], dtype=np.float32) < np.float32(threshold)
    pick = (np.asarray(select) != 0) & low[None, :]
    return np.where(pick, top2_idx[None, :, 1], top2_idx[None, :, 0])


def keymask_model(feats, Tp, stride=4, padding=0.0):
    """keymask_kernel (cassnat_task.py:328, embedding.py:121-122): frame j of the subsampled sequence is valid iff input frame
    stride * j exists and its first feature is not the padding value.  feats (B, T, F) float32 -> (B, Tp) bool."""
    feats = np.asarray(feats, np.float32)
    B, T, _ = feats.shape
    km = np.zeros((B, Tp), bool)
    for j in range(Tp):
        if stride * j < T:
            km[:, j] = feats[:, stride * j, 0] != np.float32(padding)
    return km


def expand_meta_model(rows, frames, B):
    """expand_meta_kernel: utterance b's record (frames, T', first utterance, one past the last) of the batch that holds it in the
    list of (rows, frames) batches; utterances past the list's total get the last batch's record."""
    meta = np.zeros((B, 4), np.int64)
    starts = np.concatenate([[0], np.cumsum(rows)])
    for b in range(B):
        k = min(int(np.searchsorted(starts, b, side="right")) - 1, len(rows) - 1)
        meta[b] = (frames[k], subsampled(int(frames[k])), starts[k], starts[k] + rows[k])
    return meta


def _batches(B, sub, utt_meta):
    """The reference batches of a call as index arrays: utt_meta's (any sizes), blocks of `sub`, or the whole call."""
    if utt_meta is not None:
        return [np.arange(int(m[2]), int(m[3])) for m in np.asarray(utt_meta)]
    if 0 < sub < B:
        return [np.arange((b // sub) * sub, min((b // sub) * sub + sub, B)) for b in range(B)]
    return [np.arange(B)] * B


def greedy_pack_model(tok, val, ylen, U, sos, hyp_stride, sub=0, utt_meta=None, ymax=None, row_off=None):
    """greedy_pack_kernel: the beam_width == 1 finish loop of cassnat.py:574-637 per reference batch.  A batch decoded alone has
    as many rows as its largest ylen (ylen counts the EOS row), the call has min(U, ymax if given) of them, and the hypothesis
    buffer holds hyp_stride - 1 tokens behind sos; utterance b consumes row i while i <= ylen[b].  tok / val: (B, U), or with
    row_off the packed rows (utterance b's from row_off[b] on).  Returns (hyp (B, hyp_stride) int64 zero padded, hyp_len, score)."""
    tok, val = np.asarray(tok, np.int64).reshape(-1), np.asarray(val, np.float32).reshape(-1)
    B = len(ylen)
    batches = _batches(B, sub, utt_meta)
    hyp = np.zeros((B, hyp_stride), np.int64)
    hyp_len, score = np.zeros(B, np.int64), np.zeros(B, np.float64)
    for b in range(B):
        rows_of_batch = max([0] + [int(ylen[j]) for j in batches[b]]) if (utt_meta is not None or 0 < sub < B) else U
        rows = min(rows_of_batch, U if ymax is None else min(U, int(ymax)))
        r0 = int(row_off[b]) if row_off is not None else b * U
        out, s, i = [sos], 0.0, 0
        while i < rows and i <= int(ylen[b]) and len(out) < hyp_stride:
            out.append(int(tok[r0 + i]))
            s = s + float(val[r0 + i])
            i += 1
        hyp[b, :len(out)] = out
        hyp_len[b], score[b] = len(out), s
    return hyp, hyp_len, score


def row_count_model(ylen, U, hyp_stride, sub=0, utt_meta=None, ymax=None):
    """row_plan_kernel's counts: r[b] = max(0, min(ylen[b] + 1, limit, hyp_stride - 1)) with limit = min(U, ymax if given, the
    largest ylen of b's own batch when the call holds several); row_off is their exclusive prefix sum."""
    ylen = np.asarray(ylen, np.int64)
    B = len(ylen)
    batches = _batches(B, sub, utt_meta)
    r = np.zeros(B, np.int64)
    for b in range(B):
        limit = U if ymax is None else min(U, int(ymax))
        if utt_meta is not None or 0 < sub < B:
            limit = min(limit, int(ylen[batches[b]].max(initial=0)))
        r[b] = max(0, min(int(ylen[b]) + 1, limit, hyp_stride - 1))
    return r


def row_off_model(ylen, U, hyp_stride, sub=0, utt_meta=None, ymax=None):
    return np.concatenate([[0], np.cumsum(row_count_model(ylen, U, hyp_stride, sub, utt_meta, ymax))])
