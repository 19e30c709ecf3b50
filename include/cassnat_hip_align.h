/* C ABI of the single-kernel entries of the alignment and hypothesis kernels between the encoder and the decoder side (ctc_align.hip,
 * rowops.hip): a companion of cassnat_hip.h, whose entries cn_op_ctc_align, cn_op_greedy_pack, cn_op_row_plan and cn_op_ctc_viterbi it
 * completes.  Exported by the same libraries and bound by the same parser (cassnat_asr_public_amd/abi.py: ALIGN_FUNCTIONS,
 * ALIGN_STRUCTS); one declaration per entry point.  All entries are stateless test entries: they check pointers and sizes before they
 * launch and return -1 with cn_last_error() set when they refuse; nothing is written then. */
#ifndef CASSNAT_HIP_ALIGN_H
#define CASSNAT_HIP_ALIGN_H
#include "cassnat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every form of the alignment kernel (the internal AlignArgs, field for field; all pointers device): best [B][Tp] int32, shift
 * [B][Tp], src_size / ylen [B], ymax [1], intervals [B][Tp + 1][4] (s1, e1, s2, e2 per trigger row).  src_mod > 0: keymask /
 * size_ratio / utt_meta of entry b are those of entry b % src_mod (ESA: several paths per utterance).  raw_path != 0: `best` is a
 * forced alignment's per-frame labels, not zeroed on masked frames; ylen_in [B] (may be NULL): the given label counts.  utt_meta
 * (may be NULL): [B][4] int32 as in cn_op_row_plan - entry b's own batch has utt_meta[b][1] = T' <= Tp frames: no token is carried
 * onto a frame at or past it, src_size = (ratio * T').long(), the EOS frame wraps at T'; the call reads the records back and
 * refuses a T' outside 1 .. Tp.  no_trigger != 0: every row is the entry's whole frame range and ylen / ymax carry no EOS row.
 * A Tp whose rows do not fit one workgroup's LDS (160 KiB) is refused and nothing is written.  cn_op_ctc_align is the plain form
 * of the same code.  cn_align_desc_size() is sizeof(cn_align_desc). */
typedef struct cn_align_desc {
    const int32_t* best;
    const uint8_t* keymask;
    const float* size_ratio;
    int32_t B, Tp, blank, left, right;
    int32_t src_mod;
    int32_t* shift;
    int32_t* src_size;
    int32_t* ylen;
    int32_t* ymax;
    int32_t* intervals;
    int32_t raw_path;
    const int32_t* ylen_in;
    const int32_t* utt_meta;
    int32_t no_trigger;
} cn_align_desc;
int cn_op_ctc_align_desc(const cn_align_desc* a, void* stream);
int32_t cn_align_desc_size(void);
/* The CTC greedy hypothesis as a decoder input (Transformer.fast_decode_with_ctc): the arg-max path zeroed on masked frames, repeats
 * of the previous frame's label zeroed, the non-zero labels compacted behind sos; tgt [B][ld] (ld >= Tp + 1, the rest `pad`),
 * len [B] (labels without sos), keylen [B] = len + 1, maxlen [1] = the largest len.  All pointers device. */
int cn_op_ctc_collapse(const int32_t* best, const uint8_t* keymask, int32_t B, int32_t Tp, int32_t sos, int32_t pad, int32_t ld,
                       int32_t* tgt, int32_t* len, int32_t* keylen, int32_t* maxlen, void* stream);
/* ESA sampled paths: best[g][i] = top2_idx[i][1] iff select[g][i] != 0 and expf(top2_val[i][0]) < threshold (strictly), else
 * top2_idx[i][0]; top2_idx / top2_val [M][2], select [n][M] bytes (NULL: every path is the best one), best [n][M]. */
int cn_op_esa_paths(const int32_t* top2_idx, const float* top2_val, const uint8_t* select, float threshold, int32_t* best, int32_t M,
                    int32_t n, void* stream);
/* Key mask after subsampling: keymask[b][j] = stride * j < T and feats[b][stride * j][0] != padding; feats fp32 [B][T][F],
 * keymask [B][Tp] bytes (the engine: stride 4, Tp = T' of T frames). */
int cn_op_keymask(const float* feats, int32_t B, int32_t T, int32_t F, int32_t Tp, int32_t stride, float padding, uint8_t* keymask,
                  void* stream);
/* The per-utterance records of a merged pass from its list of n batches (HOST int32 arrays, 1 <= n <= CN_MAX_SUB = 64, every entry
 * >= 1): utt_meta_dev [B][4] int32 = (frames, T' = ((frames - 1) / 2 + 1 - 1) / 2 + 1, first utterance, one past the last) of the
 * batch that holds utterance b; utterances past the sum of rows get the LAST batch's record. */
int cn_op_expand_meta(const int32_t* rows_host, const int32_t* frames_host, int32_t n, int32_t* utt_meta_dev, int32_t B, void* stream);
/* The same kernel with its row limits: utterance b's hypothesis holds n = min(ylen[b] + 1, limit, hyp_stride - 1) tokens behind sos
 * with the limit of cn_op_row_plan (sub, utt_meta_dev, ymax_dev: the same arguments, any may be 0 / NULL); row_off_dev (may be
 * NULL): b's tok / val rows start at row_off_dev[b] (cn_op_row_plan's offsets) instead of b * U.  hyp [B][hyp_stride] (zeros
 * behind the tokens), hyp_len [B] = n + 1, score [B] = the sequential double sum of the n values.  tok / val hold B * U rows.  Like
 * cn_op_ctc_align_desc, the call reads the device records it indexes by back and refuses (-1, nothing written) a utt_meta batch
 * outside 0 .. B and offsets that are not non-decreasing with 0 <= row_off_dev[b] <= b * U (what a plan of at most U rows each gives). */
int cn_op_greedy_pack_rows(const int32_t* tok, const float* val, const int32_t* ylen, int32_t B, int32_t U, int32_t sos,
                           int32_t hyp_stride, int32_t* hyp, int32_t* hyp_len, double* score, int32_t sub, const int32_t* utt_meta_dev,
                           const int32_t* ymax_dev, const int32_t* row_off_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
