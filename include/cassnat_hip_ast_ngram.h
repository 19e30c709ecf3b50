/* C ABI of the AST beam search with word n-gram shallow fusion: a companion of cassnat_hip.h, whose types it uses (cn_model,
 * cn_ngram_desc).  Exported by the same libraries and bound by the same parser (cassnat_asr_public_amd/abi.py:
 * AST_NGRAM_FUNCTIONS); one declaration per entry point. */
#ifndef CASSNAT_HIP_AST_NGRAM_H
#define CASSNAT_HIP_AST_NGRAM_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- AST beam search with word n-gram fusion (ast_ngram.hip; --task art, decode_type ctc_att, rank_model n-gram) ----------------
 * Transformer.beam_decode's search (cn_decode_ast) with an ARPA model in the place of the TransformerLM; not in the reference, whose
 * only fusion there is the TransformerLM's.
 * Words.  A live hypothesis is sos followed by tokens h.  Its text is the ranker's gluing of h: the pieces concatenated, ids equal
 * to eos left out, a separator read as a blank.  Ids outside [0, vocab) contribute no piece either.  The text's words but the last are
 * closed; the last is open unless the text ends in a blank (or is empty).  hist is <s> followed by the closed words' ids (a word
 * no model holds is <unk>, as cassnat_hip.h describes), cut to its last order - 1 entries.
 * Adds.  Per hypothesis two float32 numbers adds = (a_word, a_eos).  With close32 = score(open word | hist), the float32 sum in
 * cassnat_hip.h's order (probability, then back-off weights), and end32 = score(</s> | hist'), hist' = hist + [open word] when a
 * word is open, else hist:  a_word = close32 when a word is open, else 0;  a_eos = fl32(close32 + end32) when a word is open, else
 * end32.
 * Terms.  The term of candidate token c is a_eos if c == eos, a_word if piece_starts[c], else 0: a word is paid for when the
 * token that closes it arrives, and a hypothesis in mid-word competes without its last word's score (no lexicon look-ahead).
 * Fusion is the reference's float32 arithmetic for an LM row (transformer.py:189-214), one rounding per operation, with
 * lm_scale = float32(lm_weight * ln 10) computed in double by the caller (ARPA scores are log10):
 *   with CTC (ctc_weight > 0) the candidates are the attention top-ctc_beam as without a model, and
 *   local = fl32(local + fl32(lm_scale * term)) - cn_op_ast_beam_update's branch for use_lm with use_ctc;
 *   without CTC the candidates are the top-beam_width over the whole vocabulary of
 *   fl32(log_softmax(att / T)[c] + fl32(lm_scale * term(c))), stable descending, ties to the lower index, log_softmax as
 *   cn_op_logsoftmax_topk computes it.
 * cn_ast_attach_ngram: desc (device tables; copied by value, the tables stay the caller's and must outlive the attachment) becomes
 * the model cn_decode_ast and cn_ast_step_ngram fuse; NULL detaches, after which the handle decodes bit for bit as if nothing had
 * ever been attached.  While attached, cn_decode_ast runs [decoder step -> adds from every slot's own tokens -> top-K over the
 * vocabulary with the class terms (no CTC) or attention top-K and the terms at it (CTC) -> CTC scores -> the unchanged beam update]
 * with no host round trip; its cn_ast_opts.lm_weight must be 0.  Refused (-1, cn_last_error): a handle that is no AST model, an
 * order outside 1 .. 8, desc->vocab != the decoder's vocab_size, a slot count that is no power of two, a null table, a NaN scale.
 * An n-gram model and a TransformerLM are not fused together: cn_decode_ast with lm_weight > 0 and cn_ast_step_lm refuse while
 * an n-gram model is attached, cn_ast_step_ngram refuses while a TransformerLM is.
 * cn_op_ast_ngram_adds: adds [n][2] of the rows tok [n][ld] (row r: its first len[r] ids, clamped to [0, ld]; rows WITHOUT sos); one
 * wave per row, stateless, all pointers device.  Nothing else is written.  cn_ast_ngram_adds_host: the same step functions on the
 * host with host pointers, no GPU call; the two agree bit for bit.
 * cn_op_ast_ngram_terms: term [n][K] of the candidates idx [n][K] from adds [n][2] and starts (the desc's piece_starts); idx holds
 * ids of the vocabulary `starts` covers (a top-k's output); a negative id has term 0.
 * cn_op_logsoftmax_class_topk: per row of att [M][V] the k best of fl32(log_softmax(att / T)[c] + fl32(w * term(c))), terms from
 * adds [M][2], starts [V] and eos; 1 <= k <= min(32, V), V <= 8192; with adds all zero the output is cn_op_logsoftmax_topk's bit
 * for bit.
 * cn_ast_step_ngram: cn_ast_step with the attached model on caller-managed rows (after cn_ast_begin): adds_dev [n][2] are the
 * caller's (cn_op_ast_ngram_adds or cn_ast_ngram_adds_host).  use_ctc == 0: topk_idx_dev / topk_val_dev [n][K] are the fused top-K
 * (term_dev is not used).  use_ctc != 0: they are the attention top-K and term_dev [n][K] receives the terms at it.  eos names the
 * token whose term is a_eos (cn_ast_opts.eos of the whole search). */
int cn_ast_attach_ngram(cn_model* ast, const cn_ngram_desc* desc, float lm_scale);
int cn_op_ast_ngram_adds(const cn_ngram_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n, int32_t eos,
                         float* adds, void* stream);
int cn_ast_ngram_adds_host(const cn_ngram_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n, int32_t eos,
                           float* adds);
int cn_op_ast_ngram_terms(const uint8_t* starts, const float* adds, int32_t eos, const int32_t* idx, int32_t n, int32_t K, float* term,
                          void* stream);
int cn_op_logsoftmax_class_topk(const float* att, int32_t M, int32_t V, float temperature, const uint8_t* starts, const float* adds,
                                int32_t eos, float w, int32_t k, int32_t* idx, float* val, void* stream);
int cn_ast_step_ngram(cn_model* m, int32_t n_live, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev, const int32_t* anc_dev,
                      const uint8_t* keyok_dev, int32_t table_stride, float temperature, int32_t K, int32_t use_ctc, int32_t eos,
                      const float* adds_dev, int32_t* topk_idx_dev, float* topk_val_dev, float* term_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
