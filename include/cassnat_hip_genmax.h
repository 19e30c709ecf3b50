/* C ABI of the fused generator tail (genmax.hip): per row the arg-max, the maximum or a given target's value of
 * log_softmax(W h + b), d_model 256, without forming the logits.  A companion of cassnat_hip.h, whose entries cn_op_genmax,
 * cn_op_genmax_gather and cn_op_genmax_x3 are plain forms of cn_op_genmax_desc.  Exported by the same libraries and bound by the same
 * parser (cassnat_asr_public_amd/abi.py: GENMAX_FUNCTIONS, GENMAX_STRUCTS, GENMAX_CONSTANTS); one declaration per entry point. */
#ifndef CASSNAT_HIP_GENMAX_H
#define CASSNAT_HIP_GENMAX_H
#include "cassnat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what cn_genmax_form reports: kernel | rows << 4 | kind << 8 | vtw << 12.  kernel: the 16-bit kernel (4 waves, a quarter of the
 * vocabulary each) or the split-bf16 one (8 waves, an eighth each); rows: 32-row tiles per workgroup (1 or 2; 0: M == 0, nothing is
 * launched); kind: what a row gives; vtw: 32-entry vocabulary tiles per wave (the 16-bit kernel rounds it up to even). */
#define CN_GENMAX_KERNEL_16 0
#define CN_GENMAX_KERNEL_SPLIT 1
#define CN_GENMAX_KIND_ARGMAX_LSE 0
#define CN_GENMAX_KIND_ARGMAX 1
#define CN_GENMAX_KIND_GATHER 2

/* One launch, every field of the internal GenmaxArgs.
 *   precision  the library's own 16-bit operand (CN_PRECISION_BF16; CN_PRECISION_F16 in libcassnat_hip_f16.so) or
 *              CN_PRECISION_BF16X3 (the default library alone)
 *   h_dev      device, [M][256] in the precision's row layout: 256 16-bit operands (512 bytes), or a split-bf16 row of 1024 bytes
 *              (per 32 columns 64 bytes of bf16 hi halves, then 64 bytes of lo halves)
 *   w_host, b_host   HOST fp32 nn.Linear parameters [V][256], [V]: rounded to the operand (split-bf16: hi + lo), packed and uploaded
 *              by the call
 *   arg_dev    [M] int32: the lowest v that attains max_v (W h[m] + b)[v], as torch.argmax; maxlp_dev [M] (may be NULL: the arg-max
 *              alone, no exponentials): log_softmax(...)[arg]
 *   m_dev      NULL, or a device word with the row count of the launch, 0 <= *m_dev <= M (M sizes the grid): rows at or past it are
 *              not written, and no row of h_dev at or past it is read (a workgroup that begins at or past the count leaves at once -
 *              at a count of 0 every workgroup does; a partial workgroup reads row *m_dev - 1 in their place).  A count above M is
 *              the caller's error and is not detected.
 *   tgt_dev    NULL, or [M / U][ld] int32 targets: the call then writes tgt_lp_dev[b * ld + u] = log_softmax(W h[b * U + u] +
 *              b)[tgt_dev[b * ld + u]] for u < U and nothing else (columns U .. ld are neither read nor written).  A target outside
 *              [0, V) - negative, >= V, inside the padded tiles behind V or beyond them - gives -inf exactly; it is no error and
 *              nothing is read for it.
 * Refused (-1, cn_last_error() starts with the entry's name) before anything is sized, packed or uploaded: a null descriptor; a
 * non-zero reserved word; a precision that is neither 16-bit nor split-bf16, or that this library does not own; null h_dev, w_host
 * or b_host; M < 0; V < 1 or V > 6144; neither arg_dev nor tgt_dev; tgt_dev together with arg_dev or maxlp_dev; tgt_dev without
 * tgt_lp_dev; U < 1, ld < U or M % U != 0; maxlp_dev without arg_dev.  M == 0 returns 0 and launches nothing.
 * cn_genmax_desc_size() is sizeof(cn_genmax_desc). */
typedef struct cn_genmax_desc {
    int32_t precision;
    int32_t reserved;
    const void* h_dev;
    const float* w_host;
    const float* b_host;
    int32_t M, V;
    int32_t* arg_dev;
    float* maxlp_dev;
    const int32_t* m_dev;
    const int32_t* tgt_dev;
    int32_t U, ld;
    float* tgt_lp_dev;
} cn_genmax_desc;
int cn_op_genmax_desc(const cn_genmax_desc* d, void* stream);
int32_t cn_genmax_desc_size(void);
/* The host-only decision of the kernel such a call takes, without touching the device (no pointer is followed): the code above, or
 * -1 with the refusal ("cn_genmax_form: ...").  lds_bytes / grid (each may be NULL): the dynamic LDS of a workgroup and the number
 * of workgroups (0, 0 when nothing is launched). */
int32_t cn_genmax_form(const cn_genmax_desc* d);
int32_t cn_genmax_form_launch(const cn_genmax_desc* d, int32_t* lds_bytes, int32_t* grid);
/* Host only: the packed weight stream and bias table the kernel reads, for W [V][256] and b [V] (both HOST).
 *   16-bit:  w_out [4 waves][vtw][16 k-steps][64 lanes][8] operands - element j of lane l holds W[32 (wave * vtw + tile) + (l & 31)][16 ks
 *            + 8 (l >> 5) + j]; b_out [4 * vtw * 32] fp32
 *   split:   w_out [8][vtw][16][hi, lo][64][8] bf16 with the same lane map (hi = bf16(w), lo = bf16(w - hi)); b_out [8 * vtw * 32]
 * Vocabulary rows at or past V are zero and their biases -inf.  w_bytes / b_floats are the buffers' sizes and must be exactly
 * waves * vtw * 16384 (split: 32768) bytes and waves * vtw * 32 floats (vtw from cn_genmax_form); refused like the descriptor's
 * precision and V, and for null pointers. */
int cn_genmax_pack(int32_t precision, const float* w_host, const float* b_host, int32_t V, void* w_out, int64_t w_bytes, float* b_out,
                   int64_t b_floats);

#ifdef __cplusplus
}
#endif
#endif
