/* C ABI of the projecting form of the fused attention kernel: a companion of cassnat_hip.h, whose types it uses (cn_attn_desc).
 * Exported by the same libraries and bound by the same parser (cassnat_asr_public_amd/abi.py: PROJ_FUNCTIONS); one declaration per
 * entry point.  (cassnat_hip.h keeps the set of entry points its callers and checks count on.) */
#ifndef CASSNAT_HIP_ATTENTION_PROJ_H
#define CASSNAT_HIP_ATTENTION_PROJ_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Self attention that projects Q | K | V itself (16-bit engines; H == 4, Lq == Lk <= 256; no kv_mod / kv_index / rel_pos): y_dev
 * is LNn(x) of the B * Lq rows as cn_op_chain writes it with x_mode bit 64, wt_host [768][256] / bt_host [768] the fused Q|K|V
 * projection (host fp32, nn.Linear layout; packed on every call as the tail of a row-chain stream: a test entry point, the model
 * reads the tail units of the stream it keeps).  Q / K / V, their strides and the blocked-input fields of the descriptor are
 * unused; masks, kcap, klen, intervals, causal, scale, O / ldo / o_blocked as in cn_op_attention_desc.  O is bit for bit what
 * cn_op_chain with that projection as its tail followed by cn_op_attention_desc on the Q|K|V it wrote gives. */
int cn_op_attention_proj(int32_t precision, const cn_attn_desc* a, const void* y_dev, const float* wt_host, const float* bt_host,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
