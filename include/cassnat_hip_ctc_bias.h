/* C ABI of the CTC prefix beam search with contextual phrase biasing ("hot words"): a companion of cassnat_hip.h, whose types it uses
 * (cn_model, cn_decode_opts).  Exported by the same libraries and bound by the same parser (cassnat_asr_public_amd/abi.py:
 * CTC_BIAS_FUNCTIONS); one declaration per entry point.
 *
 * ---- Semantics -------------------------------------------------------------------------------------------------------------------
 * Phrase list (models/bias.py reads it; --hip_bias FILE): a UTF-8 text file, one phrase per line as vocabulary pieces separated by
 * blanks (the form of the token files --text_label reads, e.g. "▁new ▁york"); a line may end with a tab and a per-piece score, else
 * the phrase takes --hip_bias_score (default 3.0; natural-log units, the scale of score_ctc).  Empty lines and lines that start with
 * '#' are skipped.  Refused with the line named: a piece outside the vocabulary; blank, sos or eos in a phrase; more than 32 pieces; a
 * score that is not finite.  A duplicate phrase keeps the larger score.  No tokenizer is involved: a phrase may be listed under
 * several spellings.
 *
 * Automaton (built on the host): a trie over piece ids, node 0 the root, with Aho-Corasick failure links.  value[n] =
 * float32(depth(n)) * float32(s_n), s_n the largest per-piece score of the phrases that pass through n; value[0] = 0.  hit[n] is the
 * deepest node on the failure chain of n, n included, that ends a phrase, or -1.  Tables: an open-addressing hash table
 * (node, piece) -> child with a power-of-two slot count (probing is linear and downwards, slot - 1 modulo the slot count, from
 * hash(node, piece) & ((1 << hash_bits) - 1) & (slots - 1), hash being cb_hash of csrc/ctc_bias_search.h; a small hash_bits only
 * lengthens the probe runs and makes them wrap past slot 0); fail[n]; value[n]; bank[n] = value[hit[n]], or 0 where hit[n] is -1;
 * reset[n] = 1 where hit[n] >= 0.
 *
 * State and step: a hypothesis carries (node, banked), banked a float64; the empty hypothesis carries (0, 0.0).  A stay candidate
 * (blank, or a repetition of the last label) has its parent's state.  Appending label c to state (n, b): (1) while (n, c) has no edge
 * and n != 0, n = fail[n]; (2) take the edge if there is one, else stay at the root; (3) if reset[n'], b += double(bank[n']) and
 * n' = 0.  Every label is matched as it is (no drop_id).  score_lm of a hypothesis, and of a candidate, is banked +
 * double(value[node]); it enters the sort key (score_ctc + score_lm) + length_penalty * len(hyp) exactly where the n-gram score does.
 * After the last processed frame every kept hypothesis gives up its open match: score_lm = banked, and the beam is sorted once more
 * by the same key.  An utterance that processes no frame returns the empty hypothesis with score_lm 0.  The fail loop is bounded by
 * 32 (the longest phrase), every probe loop by its table's slot count.
 *
 * Stated limits: the shortest phrase that completes banks and restarts the match, so a phrase that properly extends another phrase
 * on the list is never completed in full.  There is no word-boundary look-ahead: "▁york" banks even if "er" follows.  The reference
 * search does not merge candidates by prefix; neither does this one.
 *
 * ---- Entry points ----------------------------------------------------------------------------------------------------------------
 * cn_ctc_beam_bias: encoder, CTC generator and per-frame pruning as cn_ctc_beam, then the whole frame loop in one launch; desc holds
 * device tables.  Outputs as cn_ctc_beam_ngram.  With opts->capture the log-posteriors are kept (cn_fetch "ctc_out").
 * cn_op_ctc_bias_beam: the kernel alone on given log-posteriors logp [B][Tp][V] and given pruned labels top_idx [B][Tp][pruning]
 * (list order is the caller's; blank and ids outside [0, V) make no candidate; may be NULL when pruning = 0); all pointers device.
 * cn_ctc_bias_beam_host: the same arguments as host pointers, no GPU call: a serial loop over the same candidate and step functions,
 * ordered by std::stable_sort (ctc_search_host of csrc/ctc_search_host.h).  It agrees with the device on hypotheses and order, on
 * score_lm bit for bit when the sums of the
 * values are exact in float64, and on the other scores up to the last bits of log1p / exp.
 * Refused without a launch (-1): a null pointer, beam outside 1 .. 32, pruning outside 0 .. 32, a slot count that is no power of
 * two, a negative node count, a null table when the node count exceeds 1, hash_bits outside 0 .. 32, B, Tp or V < 1, blank outside
 * [0, V), hyp_cap < Tp + 1, a length_penalty that is NaN.  A descriptor with the root alone (nodes <= 1) is valid: its tables are not
 * read and the search is cn_ctc_beam's with score_lm 0. */
#ifndef CASSNAT_HIP_CTC_BIAS_H
#define CASSNAT_HIP_CTC_BIAS_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cn_bias_desc {
    const int64_t* edge_keys;  /* [slots] ((int64)node << 32) | piece; -1: an empty slot */
    const int32_t* edge_child; /* [slots] */
    const int32_t* fail;       /* [nodes] */
    const float* value;        /* [nodes] */
    const float* bank;         /* [nodes] */
    const uint8_t* reset;      /* [nodes] */
    int32_t slots;
    int32_t nodes;
    int32_t hash_bits;
    int32_t reserved;
} cn_bias_desc;

int cn_ctc_beam_bias(cn_model* m, const cn_bias_desc* desc, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T,
                     int32_t F, const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty,
                     int32_t* hyp_out_dev, int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev, double* score_lm_dev,
                     double* p_blk_dev, double* p_nblk_dev, int32_t* nbeam_dev, void* stream);
int cn_op_ctc_bias_beam(const cn_bias_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                        int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp,
                        int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm, double* p_blk, double* p_nblk,
                        int32_t* nbeam, void* stream);
int cn_ctc_bias_beam_host(const cn_bias_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                          int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp,
                          int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm, double* p_blk, double* p_nblk,
                          int32_t* nbeam);

#ifdef __cplusplus
}
#endif
#endif
