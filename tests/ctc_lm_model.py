"""A numpy restatement of the CTC prefix beam search with the LM in the frame loop (src/utils/beam_decode.py:8-93 with lm_model and
args.ctc_lm_weight), in the pieces the device loop has (csrc/ctc_lm.hip): the schedule of processed frames, the frame step of one
utterance on the state of its kept hypotheses, and the whole loop around an LM callback.  tests/test_ctc_lm_model.py pins it
against the reference's own beams; tests/test_gpu_ctc_lm_kernels.py compares the kernels with it."""
import numpy as np

LOGZERO, LOGONE = -1e10, 0.0


def schedule(ctc_out, src_size, blank=0):
    """Per utterance the frames it processes: t <= src_size[b] and exp(ctc_out[b, t, blank]) (float32) <= 0.95."""
    ctc_out = np.asarray(ctc_out, np.float32)
    return [[t for t in range(ctc_out.shape[1]) if t <= int(src_size[b]) and not float(np.exp(ctc_out[b, t, blank])) > 0.95]
            for b in range(ctc_out.shape[0])]


def init_state():
    return dict(pb=np.array([LOGONE]), pnb=np.array([LOGZERO]), sctc=np.array([0.0]), slm=np.array([0.0]),
                len=np.array([0], np.int64), last=np.array([-1], np.int64))


def frame_step(st, row, top, lmrows, W, lp, lm_weight, blank=0):
    """One processed frame of one utterance.  ``st``: arrays over the kept hypotheses in list order (p_blk, p_nblk, score_ctc,
    score_lm float64; len, last int, last -1 for the empty hypothesis); ``row`` (V,) float32 log-posteriors of the frame, ``top``
    (P,) its pruned labels best first, ``lmrows`` (kept, V) float32 LM log-probabilities.  Returns (new state, parent, tok): the
    first W candidates of the stable descending sort, ``parent`` their hypothesis' list position, ``tok`` the appended label or -1.

    score_lm is a running sum that is NOT reset between the candidates of a hypothesis: float64 additions of
    double(lm log-prob) * double(lm_weight), one per non-blank pruned label, in list order."""
    cands = []
    for k in range(len(st["pb"])):
        p_b, p_nb, score_lm = float(st["pb"][k]), float(st["pnb"][k]), float(st["slm"][k])
        n, last = int(st["len"][k]), int(st["last"][k])
        new_p_nb = p_nb + float(row[last]) if n > 0 else LOGZERO
        p_temp = float(row[blank])
        new_p_b = np.logaddexp(p_b + p_temp, p_nb + p_temp)
        cands.append((new_p_b, new_p_nb, np.logaddexp(new_p_b, new_p_nb), score_lm, n, last, k, -1))
        for c in top:
            c = int(c)
            if c == blank:
                continue
            p_temp = float(row[c])
            new_p_nb = np.logaddexp(p_b + p_temp, p_nb + p_temp) if c != last else p_b + p_temp
            score_lm += float(lmrows[k][c]) * lm_weight
            cands.append((LOGZERO, new_p_nb, np.logaddexp(LOGZERO, new_p_nb), score_lm, n + 1, c, k, c))
    order = sorted(range(len(cands)), key=lambda i: cands[i][2] + cands[i][3] + lp * cands[i][4], reverse=True)[:W]
    keep = [cands[i] for i in order]
    new = dict(pb=np.array([c[0] for c in keep], np.float64), pnb=np.array([c[1] for c in keep], np.float64),
               sctc=np.array([c[2] for c in keep], np.float64), slm=np.array([c[3] for c in keep], np.float64),
               len=np.array([c[4] for c in keep], np.int64), last=np.array([c[5] for c in keep], np.int64))
    return new, np.array([c[6] for c in keep], np.int64), np.array([c[7] for c in keep], np.int64)


def fused_search(ctc_out, src_size, W, P, lp, lm_weight, lm, sos=1, blank=0):
    """The whole search: ``lm(ys (1, n) int64, mask (1, n, n) bool) -> (V,)`` gives the LM's log-probability row at the last
    position of one prefix (rows of the reference's batch are independent of each other and of its zero padding).  Returns per
    utterance the best-first list of {'hyp', 'p_blk', 'p_nblk', 'score_ctc', 'score_lm'}."""
    import torch

    ctc_out = np.asarray(ctc_out, np.float32)
    t_ctc = torch.from_numpy(ctc_out)
    top = torch.topk(t_ctc, P, dim=-1)[1].numpy() if P > 0 else np.zeros(ctc_out.shape[:2] + (0,), np.int64)
    out, rows = [], {}

    def lm_row(hyp):
        key = tuple(hyp)
        if key not in rows:
            ys = np.array([[sos] + list(hyp)], np.int64)
            n = ys.shape[1]
            mask = (ys != blank)[:, None, :] & np.tril(np.ones((n, n), bool))[None]
            rows[key] = np.asarray(lm(ys, mask), np.float32).reshape(-1)
        return rows[key]

    for b, frames in enumerate(schedule(ctc_out, src_size, blank)):
        st, hyps = init_state(), [[]]
        for t in frames:
            lmrows = [lm_row(h) for h in hyps]
            st, parent, tok = frame_step(st, ctc_out[b, t], top[b, t], lmrows, W, lp, lm_weight, blank)
            hyps = [hyps[p] + ([int(c)] if c >= 0 else []) for p, c in zip(parent, tok)]
        out.append([{"hyp": h, "p_blk": float(st["pb"][j]), "p_nblk": float(st["pnb"][j]), "score_ctc": float(st["sctc"][j]),
                     "score_lm": float(st["slm"][j])} for j, h in enumerate(hyps)])
    return out
