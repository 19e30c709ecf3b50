/* C ABI of the AST beam search with contextual phrase biasing: a companion of cassnat_hip_ctc_bias.h, whose descriptor (cn_bias_desc)
 * and phrase list it uses unchanged.  Exported by the same libraries and bound by the same parser (cassnat_asr_public_amd/abi.py:
 * AST_BIAS_FUNCTIONS); one declaration per entry point.
 *
 * ---- Semantics -------------------------------------------------------------------------------------------------------------------
 * The list, the automaton and its tables are those of cassnat_hip_ctc_bias.h (models/bias.py builds them); the search is
 * Transformer.beam_decode's (cn_decode_ast: --task art, decode_type ctc_att).  Not in the reference, which has no biasing.
 *
 * Node.  A live hypothesis is sos followed by tokens h.  Its node is the `node` component of cb_step (csrc/ctc_bias_search.h)
 * folded over h from cb_init(); a token below 0 leaves the node where it is, and with nodes <= 1 every node is the root.  Only the
 * node is carried: the search accumulates the scores itself, so `banked` is not needed.
 *
 * Term of candidate token c for a hypothesis at node n (a node outside [0, nodes) counts as the root; with nodes <= 1 every term is
 * +0.0f):
 *   c == eos              term = -value[n], and +0.0f at the root: the open match is given up when the hypothesis ends, as the CTC
 *                         search gives it up after the last frame;
 *   c < 0 or c >= V       0;
 *   otherwise             let ch be the child cb_step's walk finds (while (n, c) has no edge and n is not the root, n = fail[n], at most
 *                         32 times; every probe loop at most `slots` long; a child or failure target outside the node table counts as
 *                         the root), or the root.  Where ch != 0 and reset[ch]: gain = bank[ch], n' = 0; otherwise gain = 0, n' = ch.
 *                         term = float32((double(gain) + double(value[n'])) - double(value[n])), evaluated in that order, value[0]
 *                         taken as 0.
 * So the terms along a hypothesis plus its eos term sum to the score_lm (the banked bonus) cassnat_hip_ctc_bias.h gives the same
 * label sequence; with dyadic scores the sum is exact.
 *
 * Fusion is the reference's float32 arithmetic for an LM row (transformer.py:189-214) with the weight 1.0f:
 *   with CTC (ctc_weight > 0) the candidates are the attention top-ctc_beam, as without a list, and
 *   local = fl32(local + fl32(1.0f * term)) - cn_op_ast_beam_update's branch for use_lm with use_ctc, unchanged;
 *   without CTC the candidates are the top-beam_width over the whole vocabulary of fl32(log_softmax(att / T)[c] + term(c)), stable
 *   descending, ties to the lower index, log_softmax as cn_op_logsoftmax_topk computes it.
 *
 * Stated limits.  A hypothesis still live when max_step ends keeps the value of its open match: nothing ranks after the loop.  As in
 * the CTC search, the shortest phrase that completes banks and restarts the match, and there is no word-boundary look-ahead.  A list
 * is fused with neither a TransformerLM nor a word n-gram model.  CASS-NAT's finish loop is not biased.
 *
 * ---- Entry points ----------------------------------------------------------------------------------------------------------------
 * cn_ast_attach_bias: desc (device tables; copied by value, the tables stay the caller's and must outlive the attachment) becomes the
 * list cn_decode_ast and cn_ast_step_bias fuse; NULL detaches, after which the handle decodes bit for bit as if nothing had ever been
 * attached.  While attached, cn_decode_ast runs [decoder step -> top-K over the vocabulary with the terms (no CTC) or attention top-K
 * and the terms at it (CTC) -> CTC scores -> the unchanged beam update] with no host round trip.  It carries one node per beam slot:
 * node[pos][s] = cb_step(node[pos - 1][anc[s][pos - 1]], token of s at pos), the root at position 0, `anc` the table that names the
 * slot which computed a position (the KV cache's addressing); the launch that needs the node computes it.  cn_ast_opts.lm_weight must
 * be 0.  Refused (-1, cn_last_error): a handle that is no AST model; a slot count that is no power of two, a negative node count,
 * hash_bits outside 0 .. 32, a null table when the node count exceeds 1; an attached n-gram model
 * (cn_ast_attach_ngram refuses in turn while a list is attached).  A list and a TransformerLM are not fused together either:
 * cn_decode_ast and cn_ast_step_bias refuse while an LM is attached (cn_ast_attach_lm), cn_ast_step_lm refuses while a list is.
 * cn_op_ast_bias_nodes: node_out [n] of the rows tok [n][ld] (row r: its first len[r] ids, clamped to [0, ld]; rows WITHOUT sos); one
 * lane per row, stateless, all pointers device.  cn_ast_bias_nodes_host: the same step function on the host with host pointers, no
 * GPU call; the two agree bit for bit.
 * cn_op_ast_bias_terms: term [n][K] of the candidates idx [n][K] for the rows' nodes node [n]; one thread per (row, candidate); a
 * negative id has term 0, ids are not bounded above (a top-k's output).  cn_ast_bias_terms_host: likewise on the host.
 * cn_op_logsoftmax_bias_topk: per row of att [M][V] the k best of fl32(log_softmax(att / T)[c] + term(c)), terms of node [M];
 * 1 <= k <= min(32, V), V <= 8192; with nodes <= 1, or every node at the root of a table without edges, the output is
 * cn_op_logsoftmax_topk's bit for bit.
 * cn_ast_step_bias: cn_ast_step with the attached list on caller-managed rows (after cn_ast_begin): node_dev [n] are the caller's
 * (cn_op_ast_bias_nodes or cn_ast_bias_nodes_host).  use_ctc == 0: topk_idx_dev / topk_val_dev [n][K] are the fused top-K (term_dev
 * is not used).  use_ctc != 0: they are the attention top-K and term_dev [n][K] receives the terms at it.  eos names the token whose
 * term gives the open match up (cn_ast_opts.eos of the whole search).
 * The four cn_op_ / _host entries refuse (-1) a null pointer, n, ld, K or M < 1 and what the descriptor check refuses, and write
 * nothing then. */
#ifndef CASSNAT_HIP_AST_BIAS_H
#define CASSNAT_HIP_AST_BIAS_H
#include "cassnat_hip_ctc_bias.h"
#ifdef __cplusplus
extern "C" {
#endif

int cn_ast_attach_bias(cn_model* ast, const cn_bias_desc* desc);
int cn_op_ast_bias_nodes(const cn_bias_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n, int32_t* node_out,
                         void* stream);
int cn_ast_bias_nodes_host(const cn_bias_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n, int32_t* node_out);
int cn_op_ast_bias_terms(const cn_bias_desc* desc, const int32_t* node, int32_t eos, const int32_t* idx, int32_t n, int32_t K, float* term,
                         void* stream);
int cn_ast_bias_terms_host(const cn_bias_desc* desc, const int32_t* node, int32_t eos, const int32_t* idx, int32_t n, int32_t K,
                           float* term);
int cn_op_logsoftmax_bias_topk(const float* att, int32_t M, int32_t V, float temperature, const cn_bias_desc* desc, const int32_t* node,
                               int32_t eos, int32_t k, int32_t* idx, float* val, void* stream);
int cn_ast_step_bias(cn_model* m, int32_t n_live, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev, const int32_t* anc_dev,
                     const uint8_t* keyok_dev, int32_t table_stride, float temperature, int32_t K, int32_t use_ctc, int32_t eos,
                     const int32_t* node_dev, int32_t* topk_idx_dev, float* topk_val_dev, float* term_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
