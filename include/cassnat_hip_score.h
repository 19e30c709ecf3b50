/* C ABI of the scorer's edit alignment: a companion of cassnat_hip.h.  Exported by the same libraries and bound by the same parser
 * (cassnat_asr_public_amd/abi.py: SCORE_FUNCTIONS); one declaration per entry point, plain arguments, no struct. */
#ifndef CASSNAT_HIP_SCORE_H
#define CASSNAT_HIP_SCORE_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- weighted edit alignment of id sequences (edit_align.hip; decode_asr --hip_score, bin/score_asr) -------------------------------
 * Not in the reference, whose recipes end in sclite.  No model handle.
 * Pairs.  The call scores N pairs; pair n is ref[ref_begin[n] .. + R) against hyp[hyp_begin[n] .. + H) with R = ref_len[n] clamped to
 * [0, max_ref] and H = hyp_len[n] clamped to [0, max_hyp].  ref / hyp are int32 ids of which only equality is read (any int32 is an
 * id), the begins int64, the lengths int32.  The begins are independent of each other: pairs may share a reference.  ref_total /
 * hyp_total / ops_total are the element counts of the three buffers: a pair one of whose spans leaves its buffer (a negative begin,
 * begin + R > ref_total, begin + H > hyp_total, ops_begin + R + H > ops_total) gets cost -1, counts 0, path_len 0, and nothing is read
 * or written through it.
 * Costs c_sub, c_ins, c_del, each in 1 .. 255 (Kaldi's compute-wer: 1 / 1 / 1; sclite's DP weights: 4 / 3 / 3).
 * Definition, all in int32.  D[0][0] = 0, D[i][0] = i * c_del, D[0][j] = j * c_ins,
 *   D[i][j] = min(D[i-1][j-1] + (ref[i-1] == hyp[j-1] ? 0 : c_sub), D[i-1][j] + c_del, D[i][j-1] + c_ins).
 * The back-pointer of a cell is the first of (diagonal, up = deletion, left = insertion) that attains the minimum; row 0 points left,
 * column 0 points up.  The path is the walk from (R, H) to (0, 0) along the back-pointers.
 * Outputs per pair: cost[n] = D[R][H]; counts[n][4] = correct, substituted, deleted, inserted; path_len[n] = P;
 * ops[ops_begin[n] .. + P) the path in forward order, one uint8 per step: 0 = C, 1 = S, 2 = D, 3 = I.  The caller gives each pair
 * R + H bytes of ops; bytes behind P and rows n >= N are not written.
 * Every quantity is an integer: kernel and host entry agree exactly.
 *
 * cn_op_edit_align: all pointers device; one workgroup (one wave) per pair, rows in order, a row as prefix-minimum scans over chunks of
 * 64 hyp positions with a carry from chunk to chunk; the two live rows, the hyp ids and the back-pointers (2 bits per cell) in dynamic
 * LDS.  bp_lds_limit < 0: the back-pointers live in LDS whenever max_ref and max_hyp fit the launch's dynamic LDS, else in device
 * scratch the entry allocates and frees; bp_lds_limit >= 0: in LDS only while (max_ref + 1) * (max_hyp + 1) <= bp_lds_limit as well
 * (0 forces the scratch form).  Both forms give the same bytes.  The entry returns after the stream has drained.
 * Refused before anything is launched (-1, cn_last_error): a null buffer, N outside 1 .. 1048576, max_ref or max_hyp outside
 * 0 .. 8192, a cost outside 1 .. 255, a negative total.
 * cn_edit_align_host: the same definition, serial, every pointer a host pointer, no GPU call; built from the same step functions
 * (csrc/edit_align_search.h). */
int cn_op_edit_align(const int32_t* ref_dev, int64_t ref_total, const int64_t* ref_begin_dev, const int32_t* ref_len_dev, const int32_t* hyp_dev,
                     int64_t hyp_total, const int64_t* hyp_begin_dev, const int32_t* hyp_len_dev, int32_t N, int32_t max_ref, int32_t max_hyp,
                     int32_t c_sub, int32_t c_ins, int32_t c_del, int64_t bp_lds_limit, int32_t* cost_dev, int32_t* counts_dev,
                     int32_t* path_len_dev, uint8_t* ops_dev, int64_t ops_total, const int64_t* ops_begin_dev, void* stream);
int cn_edit_align_host(const int32_t* ref, int64_t ref_total, const int64_t* ref_begin, const int32_t* ref_len, const int32_t* hyp,
                       int64_t hyp_total, const int64_t* hyp_begin, const int32_t* hyp_len, int32_t N, int32_t max_ref, int32_t max_hyp,
                       int32_t c_sub, int32_t c_ins, int32_t c_del, int32_t* cost, int32_t* counts, int32_t* path_len, uint8_t* ops,
                       int64_t ops_total, const int64_t* ops_begin);

#ifdef __cplusplus
}
#endif
#endif
