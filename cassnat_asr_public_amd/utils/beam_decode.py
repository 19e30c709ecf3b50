"""Drop-in for the reference's ``utils.beam_decode.ctc_beam_decode`` (src/utils/beam_decode.py:8-93): CTC prefix beam search
over the encoder's log-posteriors - what ``decode_type: ctc_only`` returns and what ``decode_type: ctc_att`` aligns the NAT
decoder to (src/tasks/cassnat_task.py:335-341).

Same call and the same result - per utterance a best-first list of ``{'ys', 'p_blk', 'p_nblk', 'score_ctc', 'score_lm',
'hyp'}`` (``hyp`` without sos) - but the encoder, the CTC generator, the per-frame pruning and the whole frame loop run on
the device (``cn_ctc_beam``; csrc/ctc_beam.hip).

With ``lm_model`` a ``models.lm.TransformerLM`` and ``args.ctc_lm_weight > 0`` the reference's in-loop LM fusion runs on the
device too (``cn_ctc_beam_lm``; csrc/ctc_lm.hip): one LM step per processed frame over all kept hypotheses, ``score_lm`` the
reference's running sum over the pruned labels (it is not reset between the candidates of a hypothesis).  ``ctc_lm_weight == 0``
with an LM at hand is the LM-free search (the reference runs the LM and adds zeros).

With ``lm_model`` a ``models.ngram.NgramLM`` (``rank_model: n-gram`` with an ARPA file) the search fuses the word n-gram model
(``cn_ctc_beam_ngram``; csrc/ctc_ngram_search.h; not in the reference): a candidate whose label begins a new word adds
``ctc_lm_weight * ln(10)`` times the ARPA score of the word its parent had open, given the parent's word history; after the last
frame every hypothesis adds its open word and ``</s>``.  The whole frame loop is one launch.  Any other ``lm_model`` object - a
``kenlm.Model`` included - is refused.

With ``bias`` a ``models.bias.BiasList`` (``--hip_bias FILE``; the keyword, else ``args.hip_bias_model``) the search rewards the listed
phrases while they are being spelled (``cn_ctc_beam_bias``; include/cassnat_hip_ctc_bias.h; not in the reference): ``score_lm`` is the
banked bonus of the completed phrases plus the value of the open match, which is taken back after the last frame.  A bias list together
with a fused language model is refused.

With ``merge`` true (``--hip_ctc_merge 1``; the keyword, else ``args.hip_ctc_merge``) candidates that spell the same label sequence are
merged before they are ranked (``cn_ctc_beam_merged``; include/cassnat_hip_ctc_merge.h; not in the reference): the beam holds every
sequence once and ``score_ctc`` is a prefix probability.  It serves the LM-free, the n-gram and the bias search; together with a
TransformerLM in the loop it is refused.
"""
import math

import torch

from .. import hip
from ..models.ngram import NgramLM

logzero, logone = -1e10, 0  # src/utils/ctc_prefix.py:11-12


def ctc_beam_decode(model, src, src_mask, src_size, vocab, args, lm_model=None, engine=None, bias=None, merge=None):
    """``model``: a CassNAT (src/tasks/cassnat_task.py:335-341) or the autoregressive Transformer with its CTC head
    (src/tasks/art_task.py:252-253).  ``engine``: run on this handle (a decode pipeline's) instead of the model's own."""
    ngram = isinstance(lm_model, NgramLM)
    if lm_model is not None and not ngram and not hasattr(lm_model, "step_engine"):
        raise NotImplementedError("CTC beam search with in-loop LM fusion needs a models.lm.TransformerLM (rank_model 'lm') or a "
                                  "models.ngram.NgramLM (rank_model 'n-gram' with an ARPA file) as lm_model; %s is outside the "
                                  "accelerated path" % type(lm_model).__name__)
    if ngram and float(getattr(args, "ctc_lm_weight", 0) or 0) != 0 and not lm_model.device_ok:
        raise ValueError("a piece of the vocabulary has a separator behind its leading run: its hypotheses cannot be glued into words, "
                         "so the CTC beam search cannot fuse the n-gram model")
    if bias is None and getattr(args, "hip_bias_search", "ctc") != "att":  # (att: the list is the attention beam search's)
        bias = getattr(args, "hip_bias_model", None)
    if bias is not None and lm_model is not None and float(getattr(args, "ctc_lm_weight", 0) or 0) != 0:
        raise NotImplementedError("--hip_bias together with a language model fused into the CTC beam search (ctc_lm_weight != 0) is not "
                                  "on the accelerated path: drop one of the two")
    if merge is None:
        merge = int(getattr(args, "hip_ctc_merge", 0) or 0)
    if merge and lm_model is not None and not ngram and float(getattr(args, "ctc_lm_weight", 0) or 0) != 0:
        raise NotImplementedError("--hip_ctc_merge together with a TransformerLM fused into the CTC beam search (ctc_lm_weight != 0) is not "
                                  "on the accelerated path: that loop's score_lm is a running sum over a hypothesis' candidates and has "
                                  "no per-prefix meaning")
    if args.ctc_lp is None:
        raise TypeError("ctc_lp must be a number (with None the reference's sort key is a lambda and sorted() fails)")
    sos = vocab.word2index["sos"]
    assert vocab.word2index["blank"] == args.padding_idx, "CTC blank id and padding_idx must agree"
    dev = torch.device("cuda", getattr(model, "_device", torch.cuda.current_device()))
    feats = src.to(dev, torch.float32).contiguous()
    ratio = src_size.to(dev, torch.float32).contiguous()
    B, T, _ = feats.shape
    eng = engine if engine is not None else model.engine(B, T)
    # (args.hip_capture as in CassNAT.beam_decode: a capture run keeps every stage on the kernels that leave full tensors behind,
    # so that `ctc_out` fetched after a later call of the same engine is the tensor this search ran on)
    opts = hip.Engine.make_opts(args, capture=getattr(args, "hip_capture", False))
    opts.sos = sos
    lm_weight = float(getattr(args, "ctc_lm_weight", 0) or 0)
    slm = None
    if merge:
        kw = {}
        if bias is not None:
            if dev not in bias._dev:
                bias.cuda(dev)
            kw = dict(bias_desc=bias.desc(dev))
        elif ngram and lm_weight != 0:
            if dev not in lm_model._dev:
                lm_model.cuda(dev)
            kw = dict(ngram_desc=lm_model.desc(dev), lm_scale=lm_weight * math.log(10.0))
        hyp, hlen, sc, slm, pb, pnb, nb = eng.ctc_beam_merged(feats, ratio, opts, int(args.ctc_beam), int(args.ctc_pruning), float(args.ctc_lp),
                                                              **kw)
        slm = slm.cpu().numpy()
    elif bias is not None:
        if dev not in bias._dev:
            bias.cuda(dev)
        hyp, hlen, sc, slm, pb, pnb, nb = eng.ctc_beam_bias(bias.desc(dev), feats, ratio, opts, int(args.ctc_beam), int(args.ctc_pruning),
                                                            float(args.ctc_lp))
        slm = slm.cpu().numpy()
    elif ngram and lm_weight != 0:
        if dev not in lm_model._dev:
            lm_model.cuda(dev)
        # (ARPA scores are log10, the CTC scores natural logarithms)
        hyp, hlen, sc, slm, pb, pnb, nb = eng.ctc_beam_ngram(lm_model.desc(dev), feats, ratio, opts, int(args.ctc_beam), int(args.ctc_pruning),
                                                             float(args.ctc_lp), lm_weight * math.log(10.0))
        slm = slm.cpu().numpy()
    elif lm_model is not None and lm_weight != 0:
        lm_eng = lm_model.step_engine(B * int(args.ctc_beam))  # (one LM engine kept per model, as CassNAT._lm_finish's)
        hyp, hlen, sc, slm, pb, pnb, nb, _ = eng.ctc_beam_lm(lm_eng, feats, ratio, opts, int(args.ctc_beam), int(args.ctc_pruning),
                                                             float(args.ctc_lp), lm_weight)
        slm = slm.cpu().numpy()
    else:
        hyp, hlen, sc, pb, pnb, nb = eng.ctc_beam(feats, ratio, opts, int(args.ctc_beam), int(args.ctc_pruning), float(args.ctc_lp))
    hyp, hlen, sc, pb, pnb, nb = (t.cpu().numpy() for t in (hyp, hlen, sc, pb, pnb, nb))
    out = []
    for b in range(B):
        seqs = []
        for j in range(int(nb[b])):
            h = hyp[b, j, : hlen[b, j]].tolist()
            seqs.append({"ys": torch.tensor([[sos] + h], dtype=torch.long), "p_blk": float(pb[b, j]), "p_nblk": float(pnb[b, j]),
                         "score_ctc": float(sc[b, j]), "score_lm": float(slm[b, j]) if slm is not None else 0.0, "hyp": h})
        out.append(seqs)
    return out
