/* C ABI of the CTC prefix beam search with word n-gram fusion: the companion of cassnat_hip.h, whose types it uses (cn_model,
 * cn_decode_opts, cn_ngram_desc).  Exported by the same libraries and bound by the same parser (cassnat_asr_public_amd/abi.py:
 * EXTRA_FUNCTIONS); one declaration per entry point. */
#ifndef CASSNAT_HIP_CTC_NGRAM_H
#define CASSNAT_HIP_CTC_NGRAM_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- CTC prefix beam search with word n-gram fusion (ctc_beam.hip; decode_type ctc_only / ctc_att with rank_model n-gram) --------
 * cn_ctc_beam's search with score_lm from an ARPA model; not in the reference, whose only in-loop fusion is the TransformerLM's.  The
 * words of a hypothesis are the ones the ranker's gluing finds in its labels with drop_id = 2.  A kept hypothesis carries the carry
 * of its open word, its last 7 word ids (<s> in front) and its word count.  A stay candidate has its parent's score_lm; a candidate
 * that appends a label which begins with a separator to a parent with a non-empty open word closes that word and adds
 * double(word score) * lm_scale, the word score being the float32 sum cassnat_hip.h describes, given the parent's history; any other label
 * adds nothing.  The value derives from the parent alone (it is not cn_ctc_beam_lm's running sum over the pruned list).  The sort key
 * is (score_ctc + score_lm) + length_penalty * len(hyp), stable, descending.  After the last frame every kept hypothesis adds its
 * open word, if any, then </s>, and the beam is sorted once more by the same key; an utterance that processes no frame returns the
 * empty hypothesis with lm_scale * score(</s> | <s>).  So score_lm = lm_scale * (the word scores cn_ngram_score_host adds for the
 * hypothesis), summed in float64.  lm_scale = ctc_lm_weight * ln(10): ARPA scores are log10.  There is no lexicon look-ahead: a
 * hypothesis in mid-word competes without its last word's score.
 * cn_ctc_beam_ngram: encoder, CTC generator and per-frame pruning as cn_ctc_beam, then the whole frame loop in one launch; desc
 * holds device tables.  Outputs as cn_ctc_beam_lm.  With opts->capture the log-posteriors are kept (cn_fetch "ctc_out").
 * cn_op_ctc_ngram_beam: the kernel alone on given log-posteriors logp [B][Tp][V] and given pruned labels top_idx [B][Tp][pruning]
 * (list order is the caller's; blank and ids outside [0, V) make no candidate; may be NULL when pruning = 0); all pointers device.
 * cn_ctc_ngram_beam_host: the same arguments as host pointers, no GPU call: a serial loop over the same candidate, state-update and
 * word-score functions (ctc_search_host of csrc/ctc_search_host.h, the one loop behind every host entry).  It agrees with the
 * device on hypotheses and order, on score_lm bit for bit when the word scores are exact in float32, and on the other scores up to
 * the last bits of log1p / exp.
 * Refused without a launch (-1): a null pointer, beam outside 1 .. 32, pruning outside 0 .. 32, an order outside 1 .. 8, a slot
 * count that is no power of two, B, Tp or V < 1, blank outside [0, V), hyp_cap < Tp + 1, a length_penalty or lm_scale that is NaN. */
int cn_ctc_beam_ngram(cn_model* m, const cn_ngram_desc* desc, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T,
                      int32_t F, const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty, double lm_scale,
                      int32_t* hyp_out_dev, int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev, double* score_lm_dev,
                      double* p_blk_dev, double* p_nblk_dev, int32_t* nbeam_dev, void* stream);
int cn_op_ctc_ngram_beam(const cn_ngram_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                         int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, double lm_scale, int32_t blank,
                         int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm, double* p_blk,
                         double* p_nblk, int32_t* nbeam, void* stream);
int cn_ctc_ngram_beam_host(const cn_ngram_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                           int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, double lm_scale, int32_t blank,
                           int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm, double* p_blk,
                           double* p_nblk, int32_t* nbeam);

#ifdef __cplusplus
}
#endif
#endif
