/* C ABI of the CTC token time stamps: a companion of cassnat_hip.h, whose types it uses (cn_model, cn_decode_opts).  Exported by
 * the same libraries and bound by the same parser (cassnat_asr_public_amd/abi.py: CTC_TIMES_FUNCTIONS); one declaration per entry
 * point. */
#ifndef CASSNAT_HIP_CTC_TIMES_H
#define CASSNAT_HIP_CTC_TIMES_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- forced CTC alignment with spans and confidences (ctc_times.hip; decode_asr --hip_ctm) ----------------------------------------
 * Not in the reference, and not the aligner of decode_type ctc_att (cn_op_ctc_viterbi restates the reference's viterbi_align for the
 * trigger mask and is untouched).
 * Inputs per utterance b: float32 log-posteriors logp [B][Tp][V], frames[b] = n valid frames (clamped to [0, Tp]), labels [B][ld]
 * with label_len[b] = L of them (clamped to [0, ld]), the blank's id.
 * Definition.  States s = 0 .. 2L: even states are the blank, state 2u + 1 is label u.  All arithmetic is float64 over the float32
 * values, an impossible state is a true -inf.  Frame 0: a[0] = logp[0][blank], a[1] = logp[0][label 0], every other state -inf.
 * Frame t >= 1: a'[s] = max(a[s], a[s-1], a[s-2]) + logp[t][path[s]], the s-2 move only for odd s whose label differs from the one
 * before it; on exact ties the first of (stay, s-1, s-2) wins.  End: state 2L-1 if a[2L-1] >= a[2L], else 2L; state 0 when L = 0.
 * status[b]: 2 when one of the L labels is the blank or lies outside [0, V) (nothing is read through such a label); else 1 when no
 * path exists, which is exactly L + #{u : label u == label u-1} > n; else 0.
 * Outputs for status 0: start[b][u] / end[b][u] (end exclusive) the first and last + 1 frame the best path spends in state 2u + 1,
 * conf[b][u] the largest logp[t][label u] over that span (float32, a log-probability), score[b] the path's log-probability in
 * float64.  n = 0 and L = 0 is the empty path: score 0.  When every path has probability zero (rows holding -inf) the score is -inf,
 * the spans follow the tie rules and a label the walk never enters keeps -1 / -1 / 0.  For status 1 or 2: spans -1, conf 0, score
 * -inf.  Entries u >= L of a row and rows b >= B are not written.
 * Every step is one float64 add of exactly representable inputs: kernel and host entry agree bit for bit.
 *
 * cn_op_ctc_token_times: all pointers device; one workgroup per utterance, the two live alpha rows in float64 and the back-pointers
 * (2 bits per frame and state) in LDS.  bp_lds_limit < 0: the back-pointers live in LDS whenever Tp and ld fit the launch's dynamic
 * LDS, else in device scratch the entry allocates and frees; bp_lds_limit >= 0: in LDS only while Tp * (2 ld + 1) <= bp_lds_limit
 * as well (0 forces the scratch form).  Both forms give the same bits.  Refused before anything is launched (-1, cn_last_error): a
 * null buffer, B outside 1 .. 65536, Tp outside 1 .. 65536, V outside 1 .. 1048576, ld outside 1 .. 1500, blank outside [0, V).
 * cn_ctc_token_times_host: the same definition, serial, every pointer a host pointer, no GPU call (bp_lds_limit is not read); built
 * from the same step functions (csrc/ctc_times_search.h).
 * cn_ctc_token_times: encoder + CTC head of the handle on feats_dev [B][T][F] (the pass of cn_ctc_beam; m->logits is rewritten),
 * frames[b] = the number of set key-mask frames of utterance b (padding makes them a prefix; size_ratio_dev is not read and may be
 * NULL), blank = opts->padding_idx, then one launch.  A capture run keeps the rows as "ctc_out".  For a CASS-NAT handle and for an
 * autoregressive handle with a CTC head; an LM handle (cfg.ast = 2) and a model without a CTC head are refused.  ProfScope tag
 * "ctc_token_times". */
int cn_op_ctc_token_times(const float* logp_dev, const int32_t* frames_dev, const int32_t* labels_dev, int32_t ld, const int32_t* label_len_dev,
                          int32_t B, int32_t Tp, int32_t V, int32_t blank, int64_t bp_lds_limit, int32_t* start_dev, int32_t* end_dev,
                          float* conf_dev, double* score_dev, int32_t* status_dev, void* stream);
int cn_ctc_token_times_host(const float* logp, const int32_t* frames, const int32_t* labels, int32_t ld, const int32_t* label_len, int32_t B,
                            int32_t Tp, int32_t V, int32_t blank, int64_t bp_lds_limit, int32_t* start, int32_t* end, float* conf,
                            double* score, int32_t* status);
int cn_ctc_token_times(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                       const cn_decode_opts* opts, const int32_t* labels_dev, int32_t ld, const int32_t* label_len_dev, int32_t* start_dev,
                       int32_t* end_dev, float* conf_dev, double* score_dev, int32_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
