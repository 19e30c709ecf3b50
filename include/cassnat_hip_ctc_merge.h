/* C ABI of the CTC prefix beam search that merges candidates by prefix: a companion of cassnat_hip.h and cassnat_hip_ctc_bias.h, whose
 * types it uses (cn_model, cn_decode_opts, cn_ngram_desc, cn_bias_desc).  Exported by the same libraries and bound by the same parser
 * (cassnat_asr_public_amd/abi.py: CTC_MERGE_FUNCTIONS); one declaration per entry point.  `--hip_ctc_merge 1`.
 *
 * ---- Semantics -------------------------------------------------------------------------------------------------------------------
 * Everything of csrc/ctc_search.h holds unchanged: the frame predicate (cs_src_size, cs_skip_frame), the CTC half of a candidate
 * (cs_candidate), the sort key (cs_key), the stable top-W as a counting rank in candidate index order (candidate (k, j) of kept
 * hypothesis k and list position j, j = 0 the stay candidate, has index k * (pruning + 1) + j), and cs_write_row's output layout.
 * One step is added between forming a frame's candidates and ranking them.
 *
 * Invariant: the kept hypotheses of an utterance spell pairwise different label sequences.  It holds at the start (the one empty
 * hypothesis) and every frame keeps it.
 *
 * Duplicate labels: a label that already occurred earlier in the frame's pruned list is no candidate (par = -1), as are blank and ids
 * outside [0, V).  (A top-k never lists a label twice; the stateless entry takes hand-made lists.)
 *
 * Fold: an extension candidate (k, c) whose sequence seq(k) + c equals seq(k') of a kept hypothesis k' - that is len(k') == len(k) + 1,
 * last(k') == c and the first len(k) labels equal - is folded into the stay candidate of k':
 *     p_nblk' = cs_logaddexp(p_nblk_stay, p_nblk_ext)   (stay first)
 *     p_blk   unchanged
 *     tot'    = cs_logaddexp(p_blk, p_nblk')
 *     len, last, parent k' and tok = -1 are the stay's; the extension stops being a candidate.
 * Under the invariant (and without duplicate labels) at most one extension folds into a given stay and no two extensions spell the
 * same sequence, so nothing depends on an order of folds, and the survivors again spell pairwise different sequences: the stays spell
 * the kept sequences, the surviving extensions spell sequences that no kept hypothesis has, each once.
 *
 * Identity is of label sequences, exactly.  A hash of the sequence pre-filters and never decides.  Both implementations:
 *   host   every kept hypothesis keeps its labels as a vector; vectors are compared.
 *   device per kept hypothesis (id, pfx, hash): id is a number given when an extension is kept (step * beam + slot + 1; the empty
 *          hypothesis has 0) and inherited by stays, pfx the id of the hypothesis it extended, hash a 32-bit hash of its labels.
 *          pfx(k') == id(k) with last(k') == c proves identity (k' WAS made by appending c to the hypothesis k has been since).  The
 *          converse does not hold: a prefix can be dropped from the beam and re-created by a later extension under a new id while its
 *          old extension is still kept - links between slots alone miss that fold.  So where the ids differ and (len, last, hash)
 *          agree, both back-pointer chains are walked label by label until a label differs, both end, or they reach the same entry;
 *          every loop of the walk is bounded by the processed frames (<= T').
 *
 * Fusion policies: the n-gram state and the bias state of a hypothesis are functions of its label sequence, so a folded candidate
 * keeps the stay's state and score_lm, and its key is cs_key(tot', score_lm_stay, length_penalty, len).  The steps after the last
 * frame are unchanged (n-gram: the open word and </s>; bias: the open match is given up; one more stable sort by the same key).  The
 * TransformerLM loop (cn_ctc_beam_lm) is not merged: its score_lm is a running sum over a hypothesis' candidates and has no per-prefix
 * meaning.
 *
 * With beam 1 and pruning 0 there is nothing to fold: the search is cn_ctc_beam's.  score_ctc of a kept hypothesis is the log of
 * the summed probability of the alignments collapsing to it that the beam has not cut off - with a beam that never drops a sequence
 * and all labels in the pruned lists, of all alignments.
 *
 * ---- Entry points ----------------------------------------------------------------------------------------------------------------
 * At most one of ngram_desc / bias_desc may be set; both NULL: no fusion, score_lm 0.  lm_scale is read with ngram_desc only.
 * cn_ctc_beam_merged: encoder, CTC generator and per-frame pruning as cn_ctc_beam, then the whole frame loop in one launch;
 * descriptors hold device tables.  Outputs as cn_ctc_beam_ngram.  With opts->capture the log-posteriors are kept ("ctc_out").
 * cn_op_ctc_merged_beam: the kernel alone on given log-posteriors logp [B][Tp][V] and given pruned labels top_idx [B][Tp][pruning]
 * (list order is the caller's; may be NULL when pruning = 0); all pointers device.  cn_op_ctc_prefix_beam's outputs plus score_lm.
 * cn_ctc_merged_beam_host: the same arguments as host pointers, no GPU call: a serial loop over the same candidate and step functions,
 * ordered by std::stable_sort, identity by comparing label vectors (ctc_search_host of csrc/ctc_search_host.h with `merge` set).  It
 * agrees with the device on hypotheses and order, on score_lm
 * bit for bit when the sums are exact in float64, and on the other scores up to the last bits of log1p / exp.
 * Refused without a launch (-1): both descriptors set; and what cn_op_ctc_ngram_beam / cn_op_ctc_bias_beam refuse: a null pointer,
 * beam outside 1 .. 32, pruning outside 0 .. 32, a bad descriptor, B, Tp or V < 1, blank outside [0, V), hyp_cap < Tp + 1, a
 * length_penalty (or, with ngram_desc, lm_scale) that is NaN. */
#ifndef CASSNAT_HIP_CTC_MERGE_H
#define CASSNAT_HIP_CTC_MERGE_H
#include "cassnat_hip_ctc_bias.h"
#ifdef __cplusplus
extern "C" {
#endif

int cn_ctc_beam_merged(cn_model* m, const cn_ngram_desc* ngram_desc, double lm_scale, const cn_bias_desc* bias_desc,
                       const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                       int32_t beam, int32_t pruning, double length_penalty, int32_t* hyp_out_dev, int32_t hyp_cap,
                       int32_t* hyp_len_dev, double* score_dev, double* score_lm_dev, double* p_blk_dev, double* p_nblk_dev,
                       int32_t* nbeam_dev, void* stream);
int cn_op_ctc_merged_beam(const cn_ngram_desc* ngram_desc, double lm_scale, const cn_bias_desc* bias_desc, const float* logp,
                          const int32_t* top_idx, const float* size_ratio, int32_t B, int32_t Tp, int32_t V, int32_t beam,
                          int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len,
                          double* score, double* score_lm, double* p_blk, double* p_nblk, int32_t* nbeam, void* stream);
int cn_ctc_merged_beam_host(const cn_ngram_desc* ngram_desc, double lm_scale, const cn_bias_desc* bias_desc, const float* logp,
                            const int32_t* top_idx, const float* size_ratio, int32_t B, int32_t Tp, int32_t V, int32_t beam,
                            int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len,
                            double* score, double* score_lm, double* p_blk, double* p_nblk, int32_t* nbeam);

#ifdef __cplusplus
}
#endif
#endif
