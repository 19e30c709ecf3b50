// C-ABI of libcassnat_hip.so, the model's non-autoregressive decode paths (the handle itself is handle.hip): the encoder and
// decoder stages of CassNAT.beam_decode (reference:
// src/models/cassnat.py:420-637) and the entries built on them - greedy NAST, merged and forced passes, ESA sampling, LM scoring,
// the CTC prefix beam search and the LM-fused finish loops.
#include <algorithm>
#include <cmath>

#include "ctc_bias_search.h"  // cb_check_desc
#include "model.h"

using namespace cn_host;

namespace cn_host {

// `area`: the call may carry more utterances than max_batch (or longer ones than max_frames) as long as every buffer holds
// it (the greedy NAT decode, whose kernels take any B x T; the other entry points keep the configured bounds)
int check_call(cn_model* m, int B, int T, int F, bool area) {
    if (!m || !m->finalized) {
        cn_set_error("model not finalized");
        return -1;
    }
    if (F != m->cfg.input_size || B < 1 || T < 1 || (!area && (B > m->maxB || T > m->maxT))) {
        cn_set_error("decode: batch/frames/feature dims outside the configured workspace (B=" + std::to_string(B) +
                     " T=" + std::to_string(T) + " F=" + std::to_string(F) + ")");
        return -1;
    }
    return ws_check(m, B, T, 1, "decode");
}

// src_embed + encoder + ctc_generator + best_path_align + align_to_mask  (cassnat.py:431-468)
static int stage_encode_align(cn_model* m, const float* feats, const float* ratio, int B, int T, int F,
                              const cn_decode_opts* o, hipStream_t s) {
    CN_TRY(stage_encode(m, feats, B, T, F, o, s));
    const cn_config& c = m->cfg;
    const int Tp = m->Tp, M = B * Tp;
    const bool cap = o->capture != 0;
    // the alignment needs the arg-max only; the best path's log-probabilities are produced when a capture asks for rows
    m->ctc_maxlp_valid = cap || !m->ctc_gen.gm_w;
    CN_TRY(run_generator(m, m->ctc_gen, m->enc_h, M, m->best, m->ctc_maxlp_valid ? m->ctc_maxlp : nullptr, cap, s));
    if (cap) CN_TRY(capture(m, "ctc_out", m->logits, false, CN_DTYPE_F32, {B, Tp, c.vocab_size}, s));
    AlignArgs al;
    al.best = m->best;
    al.keymask = m->keymask;
    al.size_ratio = ratio;
    al.B = B;
    al.Tp = Tp;
    al.blank = o->padding_idx;
    al.left = o->left_trigger;
    al.right = o->right_trigger;
    al.shift = m->shift;
    al.src_size = m->src_size;
    al.ylen = m->ylen;
    al.ymax = m->ymax;
    al.intervals = m->intervals;
    al.utt_meta = m->ragged ? m->utt_meta : nullptr;
    al.no_trigger = o->no_trigger != 0;
    {
        ProfScope ps(m, "ctc_align", 0, (double)B * Tp * 9 + (double)B * (Tp + 1) * 16, s);
        CN_TRY(launch_ctc_align(al, s));
    }
    return 0;
}

// src_embed + encoder (shared by the NAST and AST paths): features -> enc_h (model precision), keymask
int stage_encode(cn_model* m, const float* feats, int B, int T, int F, const cn_decode_opts* o, hipStream_t s) {
    const cn_config& c = m->cfg;
    const int d = c.d_model;
    const int T1 = (T - 1) / 2 + 1, Tp = (T1 - 1) / 2 + 1, F1 = m->F1, F2 = m->F2;
    const int M = B * Tp;
    const bool cap = o->capture != 0;
    m->B = B;
    ++m->call_id;
    if (!m->ragged_next) m->ragged = false;  // (only cn_decode_nast_merged announces per-utterance records, for its own call)
    m->ragged_next = false;
    m->u_predicted = false;
    m->dec_group = 1;
    m->kv_ready = false;
    m->T = T;
    m->T1 = T1;
    m->Tp = Tp;
    m->U = 0;
    m->att_rows_U = 0;
    CN_TRY(launch_keymask(feats, B, T, F, Tp, 4, (float)o->padding_idx, m->keymask, s));
    // (fp16 engines: the features against the half range; split-bf16 engines: against the e4m3 range of conv2's mixed arithmetic)
    if (m->op16_fault && m->op16_feat_limit) CN_TRY(launch_feature_range(feats, (size_t)B * T * F, m->op16_feat_limit, m->op16_fault, s));
    // conv1 writes its image with a zero halo when the LDS-DMA conv2 kernel consumes it (captures want the plain image)
    // (the split-bf16 engine: two bordered bf16 planes, hi and lo, for the same kernel's X3 form)
    // (the split-bf16 engine's planes in the MIX arithmetic of conv2.hip where it applies: half-precision hi values + two e4m3 planes)
    const bool mix_planes = !cap && m->conv2_mixw && conv2_mix_applies(m->prec, d, d);
    const bool x3_planes = !mix_planes && !cap && m->conv2_x3w && conv2_x3_applies(m->prec, d, d);
    // (the fp8 engine: an e4m3 image for the same kernel's F8 form - config 5's "fp8 MFMA encoder GEMMs" include the largest one)
    // (also under capture - the accuracy of the mode is measured on captures; the e4m3 image itself is then not captured)
    const bool f8_img = m->fp8_enc && m->conv2_f8w && conv2_f8_applies(d, d);
    const bool f8_lin = f8_img && m->linear_f8w && linear256_f8_applies(d, F2 * d);  // conv2 then hands its rows on as e4m3 too
    const int halo = ((!cap && conv2_dma_applies(m->prec, d, d)) || x3_planes || mix_planes || f8_img) ? 1 : 0;
    {
        // the halo cells of the image buffer are zero already when the previous haloed image had this very shape (and nothing
        // else wrote the buffer since): conv1 then writes the interior only (halo mode 2)
        const bool same = halo && m->c1_halo_B == B && m->c1_halo_T1 == T1;
        ProfScope ps(m, "conv1", 2.0 * 9 * B * T1 * F1 * d, (double)B * T * F * 4 + (double)B * T1 * F1 * d * m->es, s);
        const UttMeta* um = m->ragged ? m->utt_meta : nullptr;
        if (mix_planes)
            CN_TRY(launch_conv1_mixplanes(feats, m->conv1_w, m->conv1_b, m->c1, B, T, F, T1, F1, d, same ? 2 : 1, std::ldexp(1.f, MIX_LG_AL),
                                          std::ldexp(1.f, MIX_LG_AQ), s, um));
        else if (x3_planes)
            CN_TRY(launch_conv1_planes(feats, m->conv1_w, m->conv1_b, m->c1, B, T, F, T1, F1, d, same ? 2 : 1, s, um));
        else if (f8_img)
            CN_TRY(launch_conv1_f8(feats, m->conv1_w, m->conv1_b, m->c1, B, T, F, T1, F1, d, same ? 2 : 1, FP8_S_IMG, s, um));
        else if (halo && m->prec == CN_PREC_BF16 && conv1_bordered_bf16_applies(d, F1))
            CN_TRY(launch_conv1_bordered_bf16(feats, m->conv1_w, m->conv1_b, m->c1, B, T, F, T1, F1, d, s, um));
        else
            CN_TRY(launch_conv1(m->prec, feats, m->conv1_w, m->conv1_b, m->c1, B, T, F, T1, F1, d, same ? 2 : halo, s, um));
        m->c1_halo_B = halo ? B : -1;
        m->c1_halo_T1 = halo ? T1 : -1;
    }
    if (cap && !f8_img) CN_TRY(capture(m, "conv1", m->c1, true, CN_DTYPE_F32, {B, T1, F1, d}, s));
    {
        GemmArgs g;
        g.A = m->c1;
        g.conv_halo = halo;
        g.W = m->conv2.W;
        g.bias = m->conv2.b;
        g.C = m->c2;
        g.ldc = d;
        g.M = M * F2;
        g.N = d;
        g.K = 9 * d;
        g.epi = CN_EPI_RELU;
        g.conv = 1;
        g.cB = B;
        g.cT1 = T1;
        g.cF1 = F1;
        g.cC = d;
        g.cT2 = Tp;
        g.cF2 = F2;
        ProfScope ps(m, "conv2", 2.0 * g.M * g.N * g.K,
                     ((double)B * T1 * F1 * d + (double)g.N * g.K + (double)g.M * g.N) * m->es, s);
        if (mix_planes) {
            const size_t wn = (size_t)d * 9 * d;
            const unsigned char* w = (const unsigned char*)m->conv2_mixw;
            CN_TRY(launch_conv2_mix(m->c1, w, w + 2 * wn, w + 3 * wn, m->conv2_mixq, m->conv2.b, m->c2, B, T1, F1, Tp, F2, s));
        } else if (x3_planes) {
            const size_t img = (size_t)B * (T1 + 2) * (F1 + 2) * d * 2, wpl = (size_t)d * 9 * d * 2;
            CN_TRY(launch_conv2_x3(m->c1, (const unsigned char*)m->c1 + img, m->conv2_x3w, (const unsigned char*)m->conv2_x3w + wpl,
                                   m->conv2.b, m->c2, B, T1, F1, Tp, F2, s));
        } else if (f8_img) {
            CN_TRY(launch_conv2_f8(m->c1, m->conv2_f8w, m->conv2_f8q, m->conv2.b, m->c2, B, T1, F1, Tp, F2, s, f8_lin ? FP8_S_IMG : 0.f));
        } else {
            CN_TRY(launch_gemm(m->prec, g, s));
        }
    }
    if (cap && !f8_lin) CN_TRY(capture(m, "conv2", m->c2, true, CN_DTYPE_F32, {B, Tp, F2, d}, s));
    if (f8_lin) {
        ProfScope ps(m, "linear_out_embed", 2.0 * M * d * (double)F2 * d, (double)M * F2 * d + (double)d * F2 * d + (double)M * d * 4, s);
        CN_TRY(launch_linear256_f8(m->c2, m->linear_f8w, m->linear_f8q, m->linear_out.b, m->x, M, F2 * d, sqrtf((float)d),
                                   c.conf_enc ? nullptr : m->pe, Tp, s));
    } else {
        GemmArgs g;
        g.A = m->c2;
        g.lda = F2 * d;
        g.W = m->linear_out.W;
        g.bias = m->linear_out.b;
        g.C = m->x;
        g.ldc = d;
        g.c_f32 = 1;
        g.M = M;
        g.N = d;
        g.K = F2 * d;
        g.epi = CN_EPI_EMBED;
        g.pe = c.conf_enc ? nullptr : m->pe;  // relative positions: x * sqrt(d) only (embedding.py:48-58, 119)
        g.pe_period = Tp;
        g.scale = sqrtf((float)d);
        ProfScope ps(m, "linear_out_embed", 2.0 * g.M * g.N * g.K,
                     ((double)g.M * g.K + (double)g.N * g.K) * m->es + (double)g.M * g.N * 4, s);
        CN_TRY(launch_gemm(m->prec, g, s));
    }
    if (cap) CN_TRY(capture(m, "x_embed", m->x, false, CN_DTYPE_F32, {B, Tp, d}, s));
    static const bool no_chain_c = cn_exp_env("CASSNAT_NO_CHAIN") != nullptr;
    if (c.conf_enc && !m->enc.empty() && m->enc[0].cf_a.w && !no_chain_c) {
        // conformer encoder on the row-chain kernel: per layer A -> relative-position attention -> B -> GLU / depthwise
        // conv / GroupNorm + Swish -> C (see pack_model, weights.hip); the residual stream stays in the blocked layout in between
        for (size_t n = 0; n < m->enc.size(); ++n) {
            const bool last = n + 1 == m->enc.size();
            const int xin = (cap || n == 0) ? 0 : CHX_IN_BLK, xout = cap ? 0 : (last ? CHX_NO_STORE : CHX_OUT_BLK);
            CN_TRY(run_conformer_layer_chain(m, m->enc[n], m->x, B, Tp, m->keymask, nullptr, false, 0, nullptr, cap, xin, xout,
                                             last ? m->enc_h : nullptr, s));
            if (cap) CN_TRY(capture(m, ("enc_layer" + std::to_string(n)).c_str(), m->x, false, CN_DTYPE_F32, {B, Tp, d}, s));
        }
        if (cap) CN_TRY(capture(m, "enc_h", m->enc_h, true, CN_DTYPE_F32, {B, Tp, d}, s));
        return 0;
    }
    if (c.conf_enc) {  // conformer encoder (fanat_conformer_blocks.py:141-170)
        for (size_t n = 0; n < m->enc.size(); ++n) {
            CN_TRY(run_conformer_self_layer(m, m->enc[n], m->x, B, Tp, m->keymask, nullptr, s));
            if (cap) CN_TRY(capture(m, ("enc_layer" + std::to_string(n)).c_str(), m->x, false, CN_DTYPE_F32, {B, Tp, d}, s));
        }
        CN_TRY(run_ln(m, m->enc_norm, m->x, m->enc_h, M, s));
        if (cap) CN_TRY(capture(m, "enc_h", m->enc_h, true, CN_DTYPE_F32, {B, Tp, d}, s));
        return 0;
    }
    static const bool no_chain = cn_exp_env("CASSNAT_NO_CHAIN") != nullptr;
    // BASELINE config 5.  With row chains (d_model 256, d_ff % 256 == 0) the feed-forward products - 80 % of a layer's
    // multiply-adds - run on e4m3 operands inside the chain kernel at twice the bf16 rate (chain.hip, F8 form) and the layer
    // goes down the bf16 engine's path below; without them, the four products of every layer as separate e4m3 launches
    if (m->fp8_enc && (m->enc_chain.size() != m->enc.size() || no_chain)) {
        for (size_t n = 0; n < m->enc.size(); ++n) {
            CN_TRY(run_enc_layer_fp8(m, m->enc[n], m->x, B, Tp, s));
            if (cap) CN_TRY(capture(m, ("enc_layer" + std::to_string(n)).c_str(), m->x, false, CN_DTYPE_F32, {B, Tp, d}, s));
        }
        CN_TRY(run_ln(m, m->enc_norm, m->x, m->enc_h, M, s));
        if (cap) CN_TRY(capture(m, "enc_h", m->enc_h, true, CN_DTYPE_F32, {B, Tp, d}, s));
        return 0;
    }
    const bool chain = !m->enc.empty() && m->enc_chain.size() == m->enc.size() && !no_chain;
    // the projections a chain launch writes for the attention kernel (Q|K|V, and the decoder side's K|V) go out in the blocked
    // layout: 1-KiB store instructions instead of thirty-two 32-byte row segments (the tail phase was store-bound)
    static const bool blk = cn_exp_env("CASSNAT_NO_BLOCKED_QKV") == nullptr;
    m->kv_blocked = false;
    // Q | K | V projected inside the attention kernel (attention.hip, PROJ): where the self-attention launch is the resident
    // 8-wave form (128 < T' <= 256, 4 heads) the chain launches in front of it end with LNn(x) - the entry launch is the
    // LayerNorm alone, layers 0 .. N - 2 run without their tail - and the attention workgroups multiply it by the tail units of
    // the same stream: the same bits, without the 3d-wide round trip.  The last launch keeps its tail (enc_h and the decoder
    // side's K|V); capture runs and cn_decode_opts.reserved[2] keep the two-launch form.
    static const bool no_attn_proj = cn_exp_env("CASSNAT_NO_ATTN_PROJ") != nullptr;
    bool proj = chain && !cap && blk && !no_attn_proj && o->reserved[2] == 0 && m->enc_entry.w && m->prec == CN_PREC_BF16 &&
                c.n_head == 4 && Tp > 128 && Tp <= 256 && m->enc_entry.tail_n == 3 * d;
    for (size_t n = 0; proj && n + 1 < m->enc_chain.size(); ++n) proj = m->enc_chain[n].tail_n == 3 * d && m->enc_chain[n].has_next;
    if (chain) {  // bf16 / d_model 256: LN + QKV of layer 0 (an entry chain launch: no FFN, x left alone), then per layer
                  // attention -> row-chain kernel
        if (m->enc_entry.w && proj) {
            CN_TRY(run_chain(m, m->enc_entry, m->x, M, m->xn, d, true, CHX_NO_STORE, s, nullptr, 0, false, "row_chain", nullptr, true));
        } else if (m->enc_entry.w) {
            CN_TRY(run_chain(m, m->enc_entry, m->x, M, m->qkv, 3 * d, true, CHX_NO_STORE, s, nullptr, 0, blk));
        } else {
            CN_TRY(run_ln(m, m->enc[0].n[0], m->x, m->xn, M, s));
            CN_TRY(run_linear(m, "qkv_proj", m->enc[0].qkv, m->xn, d, m->qkv, 3 * d, 0, M, 0, nullptr, 0, s));
        }
    }
    // split-bf16 engine: every encoder layer in the row-chain form (all layers or none: the Q|K|V hand-over is layer to layer)
    static const bool no_x3_chain = cn_exp_env("CASSNAT_NO_X3_CHAIN") != nullptr;
    bool x3_rows = !chain && !cap && !no_x3_chain && m->prec == CN_PREC_X3 && !m->enc.empty() && m->enc[0].qkv.px3;
    for (size_t n = 0; x3_rows && n < m->enc.size(); ++n)
        x3_rows = x3_chain_applies(m, m->enc[n], n + 1 < m->enc.size() ? &m->enc[n + 1].qkv : nullptr);
    for (size_t n = 0; n < m->enc.size(); ++n) {
        const Layer& L = m->enc[n];
        const bool last = n + 1 == m->enc.size();
        if (chain) {
            if (proj)  // (the tail that projects layer n's Q|K|V: the entry stream's, then layer n - 1's)
                CN_TRY(run_self_attn_core(m, B, Tp, m->keymask, nullptr, 0, s, false, nullptr, n > 0 ? &m->enc_chain[n - 1] : &m->enc_entry));
            else
                CN_TRY(run_self_attn_core(m, B, Tp, m->keymask, nullptr, 0, s, (n > 0 || m->enc_entry.w) && blk));
            // between chain launches the residual stream lives in the kernel's blocked layout; the last layer's x is
            // consumed by nobody (enc_h is the output).  Captures read x row-major.
            const int xm = cap ? 0 : ((n > 0 ? CHX_IN_BLK : 0) | (last ? CHX_NO_STORE : CHX_OUT_BLK));
            if (last && m->kv_cols > 0) {  // enc_h and, from the same registers, every decoder-side layer's K|V
                CN_TRY(run_chain(m, m->enc_chain[n], m->x, M, m->kv_all, m->kv_cols, true, xm, s, m->enc_h, d, blk));
                m->kv_ready = true;
                m->kv_blocked = blk;
            } else if (proj && !last) {
                CN_TRY(run_chain(m, m->enc_chain[n], m->x, M, m->xn, d, true, xm, s, nullptr, 0, false, "row_chain", nullptr, true));
            } else {
                CN_TRY(run_chain(m, m->enc_chain[n], m->x, M, last ? m->enc_h : m->qkv, last ? d : 3 * d, true, xm, s, nullptr, 0,
                                 blk && !last));
            }
        } else if (x3_rows) {
            // split-bf16 engine: attention, then ONE launch for the out-projection, the feed-forward sublayer and the next layer's
            // Q|K|V (the last layer: enc_h).  (A capture run keeps the unfused kernels: the fused path's reference in the tests.)
            if (n == 0) {
                CN_TRY(run_ln(m, L.n[0], m->x, m->xn, M, s));
                CN_TRY(run_linear(m, "qkv_proj", L.qkv, m->xn, d, m->qkv, 3 * d, 0, M, 0, nullptr, 0, s));
            }
            CN_TRY(run_self_attn_core(m, B, Tp, m->keymask, nullptr, 0, s));
            if (last)
                CN_TRY(run_x3_chain(m, L, L.n[1], m->x, M, m->enc_norm, m->enc_h, nullptr, nullptr, 0, "row_chain_x3", s));
            else
                CN_TRY(run_x3_chain(m, L, L.n[1], m->x, M, m->enc[n + 1].n[0], nullptr, &m->enc[n + 1].qkv, m->qkv, 3 * d, "row_chain_x3", s));
        } else {
            CN_TRY(run_self_attn(m, L, n == 0 ? &L.n[0] : nullptr, m->x, B, Tp, m->keymask, nullptr, 0, s));
            CN_TRY(run_ffn(m, L, L.n[1], m->x, M, last ? &m->enc_norm : &m->enc[n + 1].n[0], last ? m->enc_h : m->xn, s));
        }
        if (cap) CN_TRY(capture(m, ("enc_layer" + std::to_string(n)).c_str(), m->x, false, CN_DTYPE_F32, {B, Tp, d}, s));
    }
    if (m->enc.empty()) CN_TRY(run_ln(m, m->enc_norm, m->x, m->enc_h, M, s));
    if (cap) CN_TRY(capture(m, "enc_h", m->enc_h, true, CN_DTYPE_F32, {B, Tp, d}, s));
    return 0;
}

// acembed_extractor + embed_mapper + decoder + att_generator + greedy finish  (cassnat.py:475-497, 574-637)
static int stage_decode_tail(cn_model* m, int U, const cn_decode_opts* o, int32_t* hyp, int hyp_stride, int32_t* hyp_len,
                             double* score, hipStream_t s);

static int stage_decode(cn_model* m, int U, const cn_decode_opts* o, int32_t* hyp, int hyp_stride, int32_t* hyp_len,
                        double* score, hipStream_t s) {
    const cn_config& c = m->cfg;
    const int d = c.d_model, B = m->B * m->dec_group, Tp = m->Tp, MU = B * U;
    const bool cap = o->capture != 0;
    m->U = U;
    if (U > m->pe_rows || U < 1 || U > Tp + 1) {
        cn_set_error("decode: token count exceeds the positional table / the frames of the batch");
        return -1;
    }
    // every decoder-side buffer against B x alignments-per-utterance x rows (host-side, before anything is launched)
    CN_TRY(ws_check(m, m->B, m->T, m->dec_group, "decoder side"));
    const bool uni = o->use_unimask != 0;
    // Packed decoder rows: on the greedy row-chain path every utterance owns only the rows its hypothesis reads -
    // launch_row_plan's r[b], one utterance behind the other - instead of U rows; nothing reads the rest.  The capacity stays
    // B x U (the grids are sized by it); the row kernels take the true count from row_off[B] on the device, the attention
    // launches the per-utterance windows from row_off.  cn_decode_opts.reserved[1] asks for the padded layout.  (use_trigger
    // off stays padded: an utterance without any token then has every key masked and attends uniformly over the U padded rows.)
    static const bool no_chain_p = cn_exp_env("CASSNAT_NO_CHAIN") != nullptr;
    const bool packed = !c.conf_dec && !m->dec_steps.empty() && !no_chain_p && hyp && !cap && !uni && o->beam_width == 1 &&
                        o->reserved[0] == 0 && o->reserved[1] == 0 && !o->no_trigger && m->dec_group == 1;
    m->rows_packed = packed;
    const int* roff = packed ? m->row_off : nullptr;
    const int* rows_dev = packed ? m->row_off + B : nullptr;
    if (packed) {
        CN_TRY(launch_row_plan(m->ylen, B, U, hyp_stride, o->sub_batch, m->ragged ? m->utt_meta : nullptr,
                               m->u_predicted ? m->ymax : nullptr, m->row_off, s));
        CN_TRY(launch_fill_queries_packed(m->pe, m->xd, m->row_off, B, MU, d, s));
    } else {
        CN_TRY(launch_fill_queries(m->pe, m->xd, B, U, d, s));
    }
    // The LayerNorm that follows an FFN is produced by that FFN (-> m->xn); `pending` says whether the next
    // sublayer may skip its own LayerNorm.  use_unimask shifts the stream between SAD and MAD, so no carry there.
    auto first_norm_after = [&](int stage, size_t idx) -> const Norm* {  // stage 0 extractor, 1 SAD, 2 MAD
        if (stage == 0 && idx + 1 < m->extra.size()) return &m->extra[idx + 1].n[0];
        if (stage <= 0 && !m->sad.empty()) return &m->sad[0].n[0];
        if (stage == 1 && idx + 1 < m->sad.size()) return &m->sad[idx + 1].n[0];
        if (stage <= 1) return (uni || m->mad.empty()) ? nullptr : &m->mad[0].n[0];
        if (idx + 1 < m->mad.size()) return &m->mad[idx + 1].n[0];
        return nullptr;
    };
    if (c.conf_dec) {
        if (uni) {
            cn_set_error("decode: use_unimask is not defined for the conformer decoder (the reference indexes a tuple there)");
            return -1;
        }
        float* x = m->xd;
        // ConAcExtra (fanat_conformer_blocks.py:41-60, 172-186): attention on the raw position queries, output projection
        // WITHOUT residual or pre-norm, scaled by sqrt(d); then x += FFN_swish(LN x)
        for (size_t i = 0; i < m->extra.size(); ++i) {
            const Layer& L = m->extra[i];
            CN_TRY(launch_convert(m->prec, x, m->xn, (size_t)MU * d, s));
            CN_TRY(run_linear(m, "src_q_proj", L.src_q, m->xn, d, m->qd, d, 0, MU, 0, nullptr, 0, s));
            CN_TRY(run_src_attn_core(m, L, B, U, Tp, m->intervals, s));
            {
                ProfScope ps(m, "out_proj_scaled", 2.0 * MU * d * d, (double)MU * d * (m->es + 4), s);
                GemmArgs g;
                g.A = m->ctx;
                g.lda = d;
                g.W = L.src_o.W;
                g.bias = L.src_o.b;
                g.C = x;
                g.ldc = d;
                g.c_f32 = 1;
                g.M = MU;
                g.N = d;
                g.K = d;
                g.epi = CN_EPI_EMBED;
                g.pe = nullptr;
                g.scale = sqrtf((float)d);
                CN_TRY(launch_gemm(m->prec, g, s));
            }
            CN_TRY(run_ffn_swish(m, L.w1, L.w2, L.n[0], x, MU, 1.0f, s));
        }
        if (cap) CN_TRY(capture(m, "ac_embed", x, false, CN_DTYPE_F32, {B, U, d}, s));
        static const bool no_chain_d = cn_exp_env("CASSNAT_NO_CHAIN") != nullptr;
        const bool dchain = !no_chain_d && ((!m->sad.empty() && m->sad[0].cf_a.w) || (!m->mad.empty() && m->mad[0].cf_a.w));
        if (dchain) {
            // the self- and mixed-attention conformer layers on the row-chain kernel (the extractor above stays generic);
            // the stream is row-major where something else reads it (extractor output, the pred_embed capture), blocked otherwise
            const size_t ns = m->sad.size(), nm = m->mad.size();
            for (size_t i = 0; i < ns + nm; ++i) {
                const bool mixed = i >= ns, last = i + 1 == ns + nm;
                const Layer& L = mixed ? m->mad[i - ns] : m->sad[i];
                const bool rm_in = cap || i == 0, rm_out = cap;
                const int xin = rm_in ? 0 : CHX_IN_BLK, xout = last ? CHX_NO_STORE : (rm_out ? 0 : CHX_OUT_BLK);
                CN_TRY(run_conformer_layer_chain(m, L, x, B, U, nullptr, m->ylen, mixed, Tp, o->src_trigger ? m->intervals : nullptr,
                                                 cap, xin, xout, last ? m->dec_h : nullptr, s));
                if (cap && !mixed && i + 1 == ns) CN_TRY(capture(m, "pred_embed", x, false, CN_DTYPE_F32, {B, U, d}, s));
            }
            if (cap && ns == 0) CN_TRY(capture(m, "pred_embed", x, false, CN_DTYPE_F32, {B, U, d}, s));
            if (ns + nm == 0) CN_TRY(run_ln(m, m->dec_norm, x, m->dec_h, MU, s));
            return stage_decode_tail(m, U, o, hyp, hyp_stride, hyp_len, score, s);
        }
        for (size_t i = 0; i < m->sad.size(); ++i) CN_TRY(run_conformer_self_layer(m, m->sad[i], x, B, U, nullptr, m->ylen, s));
        if (cap) CN_TRY(capture(m, "pred_embed", x, false, CN_DTYPE_F32, {B, U, d}, s));
        for (size_t i = 0; i < m->mad.size(); ++i) {  // MixAttLayer, relative branch (:85-97)
            const Layer& L = m->mad[i];
            CN_TRY(run_ffn_swish(m, L.w1, L.w2, L.n[0], x, MU, 0.5f, s));
            CN_TRY(run_rel_self_attn(m, L, L.n[2], x, B, U, nullptr, m->ylen, s));
            CN_TRY(run_conv_module(m, L, L.n[1], x, B, U, s));
            CN_TRY(run_src_attn(m, L, &L.n[3], x, B, U, Tp, o->src_trigger ? m->intervals : nullptr, s));
            CN_TRY(run_ffn_swish(m, L.ff2_w1, L.ff2_w2, L.n[4], x, MU, 0.5f, s));
        }
        CN_TRY(run_ln(m, m->dec_norm, x, m->dec_h, MU, s));
        return stage_decode_tail(m, U, o, hyp, hyp_stride, hyp_len, score, s);
    }
    static const bool no_chain = cn_exp_env("CASSNAT_NO_CHAIN") != nullptr;
    if (!m->dec_steps.empty() && !no_chain) {
        // bf16 / d_model 256: every sublayer is [attention] + one row-chain launch that also produces the next
        // sublayer's input projection (src Q -> m->qd, self Q|K|V -> m->qkv) or, after the last one, dec_h
        float* xdec = m->xd;
        const size_t n = m->dec_steps.size();
        auto proj_out = [&](const DecStep& st, void*& out, int& ldo) {
            out = st.self ? m->qkv : m->qd;
            ldo = st.self ? 3 * d : d;
        };
        for (size_t k = 0; k < n; ++k) {
            const DecStep& st = m->dec_steps[k];
            const Layer& L = st.stack == 0 ? m->extra[st.layer] : st.stack == 1 ? m->sad[st.layer] : m->mad[st.layer];
            const bool first_mad = st.stack == 2 && st.layer == 0 && st.self;
            if (first_mad) {
                if (cap) CN_TRY(capture(m, "pred_embed", m->xd, false, CN_DTYPE_F32, {B, U, d}, s));
                if (uni) {
                    CN_TRY(launch_shift_right(m->xd, m->xd2, B, U, d, s));
                    xdec = m->xd2;
                }
            }
            static const bool blkd = cn_exp_env("CASSNAT_NO_BLOCKED_QKV") == nullptr;
            if (k == 0 || (first_mad && uni)) {
                void* out;
                int ldo;
                proj_out(st, out, ldo);
                CN_TRY(run_chain(m, st.entry, xdec, MU, out, ldo, true, CHX_NO_STORE, s, nullptr, 0, blkd, "row_chain_dec", rows_dev));  // reads row-major x, writes none
            }
            if (st.self)
                CN_TRY(run_self_attn_core(m, B, U, nullptr, m->ylen, (st.stack == 2 && uni) ? 1 : 0, s, blkd, roff));
            else
                CN_TRY(run_src_attn_core(m, L, B, U, Tp,
                                         st.stack == 0 ? m->intervals : (o->src_trigger ? m->intervals : nullptr), s, blkd, roff));
            const bool final = k + 1 == n;
            // use_unimask shifts the stream between the last SAD layer and the first MAD layer: nothing carries over
            const bool carry = final || !(uni && m->dec_steps[k + 1].stack == 2 && m->dec_steps[k + 1].layer == 0 &&
                                          m->dec_steps[k + 1].self);
            void* out = m->dec_h;
            int ldo = d;
            if (!final) proj_out(m->dec_steps[k + 1], out, ldo);
            // blocked between chain launches; row-major where something else touches the stream (queries in, the
            // use_unimask shift, captures); the last sublayer's x is consumed by nobody
            const bool in_rm = k == 0 || (first_mad && uni);
            const bool out_rm = !final && !carry;
            const int xm = cap ? 0 : ((in_rm ? 0 : CHX_IN_BLK) | (final ? CHX_NO_STORE : (out_rm ? 0 : CHX_OUT_BLK)));
            CN_TRY(run_chain(m, st.chain, xdec, MU, out, ldo, carry, xm, s, nullptr, 0, blkd && !final, "row_chain_dec", rows_dev));
            if (cap && st.stack == 0 && (k + 1 == n || m->dec_steps[k + 1].stack != 0))
                CN_TRY(capture(m, "ac_embed", m->xd, false, CN_DTYPE_F32, {B, U, d}, s));
        }
        if (cap && m->mad.empty()) CN_TRY(capture(m, "pred_embed", m->xd, false, CN_DTYPE_F32, {B, U, d}, s));
        return stage_decode_tail(m, U, o, hyp, hyp_stride, hyp_len, score, s);
    }
    bool pending = false;
    for (size_t i = 0; i < m->extra.size(); ++i) {
        const Layer& L = m->extra[i];
        CN_TRY(run_src_attn(m, L, pending ? nullptr : &L.n[0], m->xd, B, U, Tp, m->intervals, s));
        const Norm* nx = first_norm_after(0, i);
        CN_TRY(run_ffn(m, L, L.n[1], m->xd, MU, nx, m->xn, s));
        pending = nx != nullptr;
    }
    if (cap) CN_TRY(capture(m, "ac_embed", m->xd, false, CN_DTYPE_F32, {B, U, d}, s));
    for (size_t i = 0; i < m->sad.size(); ++i) {
        const Layer& L = m->sad[i];
        CN_TRY(run_self_attn(m, L, pending ? nullptr : &L.n[0], m->xd, B, U, nullptr, m->ylen, 0, s));
        const Norm* nx = first_norm_after(1, i);
        CN_TRY(run_ffn(m, L, L.n[1], m->xd, MU, nx, m->xn, s));
        pending = nx != nullptr;
    }
    if (cap) CN_TRY(capture(m, "pred_embed", m->xd, false, CN_DTYPE_F32, {B, U, d}, s));
    float* xdec = m->xd;
    if (uni) {
        CN_TRY(launch_shift_right(m->xd, m->xd2, B, U, d, s));
        xdec = m->xd2;
        pending = false;
    }
    for (size_t i = 0; i < m->mad.size(); ++i) {
        const Layer& L = m->mad[i];
        const bool last = i + 1 == m->mad.size();
        CN_TRY(run_self_attn(m, L, pending ? nullptr : &L.n[0], xdec, B, U, nullptr, m->ylen, uni ? 1 : 0, s));
        CN_TRY(run_src_attn(m, L, &L.n[1], xdec, B, U, Tp, o->src_trigger ? m->intervals : nullptr, s));
        const Norm* nx = last ? &m->dec_norm : first_norm_after(2, i);
        CN_TRY(run_ffn(m, L, L.n[2], xdec, MU, nx, last ? m->dec_h : m->xn, s));
        pending = !last && nx != nullptr;
    }
    if (m->mad.empty()) CN_TRY(run_ln(m, m->dec_norm, xdec, m->dec_h, MU, s));
    return stage_decode_tail(m, U, o, hyp, hyp_stride, hyp_len, score, s);
}

// generator + argmax / top-k + hypothesis packing on m->dec_h
static int stage_decode_tail(cn_model* m, int U, const cn_decode_opts* o, int32_t* hyp, int hyp_stride, int32_t* hyp_len,
                             double* score, hipStream_t s) {
    const cn_config& c = m->cfg;
    const int d = c.d_model, B = m->B * m->dec_group, MU = B * U;
    const bool cap = o->capture != 0;
    if (cap) CN_TRY(capture(m, "dec_h", m->dec_h, true, CN_DTYPE_F32, {B, U, d}, s));
    const int k = o->beam_width;
    const bool keep_rows = o->reserved[0] != 0;  // cn_decode_opts.reserved[0]: the LM-fused finish reads the full rows at any beam width
    // (packed rows: the fused generator takes the row count from the device; tok / val are packed as dec_h is)
    CN_TRY(run_generator(m, m->att_gen, m->dec_h, MU, m->tok, m->val, cap || k > 1 || keep_rows, s,
                         m->rows_packed ? m->row_off + B : nullptr));
    // (a merged / coalesced / row-predicted pass is not offered to cn_nat_lm_finish: its utterances count their rows per batch)
    const bool plain_pass = m->dec_group == 1 && !m->ragged && !m->u_predicted && o->sub_batch == 0;
    m->att_rows_U = (cap || k > 1 || keep_rows) && plain_pass ? U : 0;
    if (cap) CN_TRY(capture(m, "att_out", m->logits, false, CN_DTYPE_F32, {B, U, c.vocab_size}, s));
    m->last_k = 0;
    if (k > 1) {
        CN_TRY(launch_topk(m->logits, MU, c.vocab_size, c.vocab_size, k, m->topk_idx, m->topk_val, s));
        m->last_k = k;
    }
    if (hyp)
        CN_TRY(launch_greedy_pack(m->tok, m->val, m->ylen, B, U, o->sos, hyp_stride, hyp, hyp_len, score, s, o->sub_batch,
                                  m->ragged ? m->utt_meta : nullptr, m->u_predicted ? m->ymax : nullptr,
                                  m->rows_packed ? m->row_off : nullptr));
    return 0;
}

}  // namespace cn_host

extern "C" int cn_encode_align(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T,
                               int32_t F, const cn_decode_opts* opts, int32_t* ymax_host, void* stream) {
    CN_TRY(check_call(m, B, T, F));
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(stage_encode_align(m, feats_dev, size_ratio_dev, B, T, F, opts, s));
    CN_HIP_CHECK(hipMemcpyAsync(m->ymax_pinned, m->ymax, sizeof(int), hipMemcpyDeviceToHost, s));
    CN_HIP_CHECK(hipStreamSynchronize(s));
    const int ymax = *m->ymax_pinned;
    if (ymax_host) *ymax_host = ymax;
    return 0;
}

namespace cn_host {
namespace {
// greedy NAT decode of one call; subs != null: a merged pass (see cn_decode_nast_merged); u_hint > 0: predicted row count
int decode_nast_impl(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                     const cn_decode_opts* opts, const SubList* subs, int32_t u_hint, int32_t* hyp_out_dev, int32_t hyp_stride,
                     int32_t* hyp_len_dev, double* score_dev, void* stream, int32_t* ticket_out) {
    CN_TRY(check_call(m, B, T, F, /*area=*/true));
    if (!opts || opts->beam_width < 1 || opts->beam_width > 16) {
        cn_set_error("cn_decode_nast: beam_width must be in [1,16]");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));  // callers may decode from several host threads (one handle each)
    if (subs) {
        if (m->cfg.conf_enc || m->cfg.conf_dec) {
            cn_set_error("cn_decode_nast_merged: transformer blocks only (a conformer's GroupNorm sees the padded rows of the merged pass)");
            return -1;
        }
        if (opts->capture || opts->beam_width != 1 || opts->sub_batch) {
            cn_set_error("cn_decode_nast_merged: greedy decode without capture; sub_batch is implied by the batch list");
            return -1;
        }
        CN_TRY(launch_expand_meta(*subs, m->utt_meta, B, s));
        m->ragged = true;
        m->ragged_next = true;
    }
    CN_TRY(stage_encode_align(m, feats_dev, size_ratio_dev, B, T, F, opts, s));
    const int slot = (int)(m->ticket_seq & 3);
    if (u_hint > 0 && opts->beam_width == 1 && !opts->capture) {
        // No mid-pass host sync: the decoder side is launched on the predicted row count.  Results do not depend on U as long
        // as U >= the true maximum (rows past an utterance's own count are masked keys that contribute exactly zero, and the
        // finish is limited by the device-side counts); the true maximum lands in the ticket's page-locked word and the caller
        // checks it once the stream has drained (cn_decode_ticket) - on a miss the pass is decoded again.
        const int U = std::min(std::max(u_hint, 1), m->Tp + 1);
        if (hyp_out_dev && hyp_stride < U + 1) {
            cn_set_error("cn_decode_nast: hyp_stride " + std::to_string(hyp_stride) + " < predicted rows + 1 = " + std::to_string(U + 1));
            return -1;
        }
        m->u_predicted = true;
        CN_HIP_CHECK(hipMemcpyAsync(m->ymax_ring + slot, m->ymax, sizeof(int), hipMemcpyDeviceToHost, s));
        m->ticket_U[slot] = U;
        CN_TRY(stage_decode(m, U, opts, hyp_out_dev, hyp_stride, hyp_len_dev, score_dev, s));
    } else {
        CN_HIP_CHECK(hipMemcpyAsync(m->ymax_ring + slot, m->ymax, sizeof(int), hipMemcpyDeviceToHost, s));
        CN_HIP_CHECK(hipStreamSynchronize(s));  // U is data dependent
        const int ymax = m->ymax_ring[slot];
        *m->ymax_pinned = ymax;
        if (ymax < 1 || ymax > m->Tp + 1) {
            cn_set_error("cn_decode_nast: alignment produced an impossible token count");
            return -3;
        }
        if (hyp_out_dev && hyp_stride < ymax + 1) {
            cn_set_error("cn_decode_nast: hyp_stride " + std::to_string(hyp_stride) + " < ymax+1 = " + std::to_string(ymax + 1));
            return -1;
        }
        m->ticket_U[slot] = ymax;
        CN_TRY(stage_decode(m, ymax, opts, hyp_out_dev, hyp_stride, hyp_len_dev, score_dev, s));
    }
    // a ticket is the call's sequence number (its word is seq & 3): cn_decode_ticket can tell a word that a later call on this
    // handle - cn_decode_nast included - has taken over, instead of handing out another pass's counts
    m->ticket_id[slot] = (int)(m->ticket_seq & 0x3fffffff);
    if (ticket_out) *ticket_out = m->ticket_id[slot];
    ++m->ticket_seq;
    return 0;
}
}  // namespace
}  // namespace cn_host

extern "C" int cn_decode_nast(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T,
                              int32_t F, const cn_decode_opts* opts, int32_t* hyp_out_dev, int32_t hyp_stride,
                              int32_t* hyp_len_dev, double* score_dev, void* stream) {
    return decode_nast_impl(m, feats_dev, size_ratio_dev, B, T, F, opts, nullptr, 0, hyp_out_dev, hyp_stride, hyp_len_dev, score_dev,
                            stream, nullptr);
}

extern "C" int cn_decode_nast_merged(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                                     const cn_decode_opts* opts, int32_t n_sub, const int32_t* sub_rows_host,
                                     const int32_t* sub_frames_host, int32_t u_hint, int32_t* hyp_out_dev, int32_t hyp_stride,
                                     int32_t* hyp_len_dev, double* score_dev, void* stream, int32_t* ticket_out) {
    if (n_sub < 0 || n_sub > CN_MAX_SUB || (n_sub > 0 && (!sub_rows_host || !sub_frames_host))) {
        cn_set_error("cn_decode_nast_merged: between 0 and " + std::to_string(CN_MAX_SUB) + " batches per pass");
        return -1;
    }
    if (n_sub == 0)
        return decode_nast_impl(m, feats_dev, size_ratio_dev, B, T, F, opts, nullptr, u_hint, hyp_out_dev, hyp_stride, hyp_len_dev,
                                score_dev, stream, ticket_out);
    SubList subs;
    subs.n = n_sub;
    long long rows = 0;
    for (int k = 0; k < n_sub; ++k) {
        if (sub_rows_host[k] < 1 || sub_frames_host[k] < 1 || sub_frames_host[k] > T) {
            cn_set_error("cn_decode_nast_merged: every batch needs >= 1 utterance and 1 <= frames <= T");
            return -1;
        }
        subs.rows[k] = sub_rows_host[k];
        subs.frames[k] = sub_frames_host[k];
        rows += sub_rows_host[k];
    }
    if (rows != B) {
        cn_set_error("cn_decode_nast_merged: the batches' utterance counts must add up to B");
        return -1;
    }
    return decode_nast_impl(m, feats_dev, size_ratio_dev, B, T, F, opts, &subs, u_hint, hyp_out_dev, hyp_stride, hyp_len_dev, score_dev,
                            stream, ticket_out);
}

extern "C" int cn_decode_ticket(cn_model* m, int32_t ticket, int32_t* ymax_host, int32_t* rows_used_host) {
    if (!m || !m->ymax_ring || ticket < 0) {
        cn_set_error("cn_decode_ticket: bad ticket");
        return -1;
    }
    const int slot = ticket & 3;
    if (m->ticket_id[slot] != ticket) {
        cn_set_error("cn_decode_ticket: ticket " + std::to_string(ticket) + " has expired - more than three decode calls were started on "
                     "this handle since it was issued (at most four passes may be outstanding per handle)");
        return -1;
    }
    if (ymax_host) *ymax_host = m->ymax_ring[slot];
    if (rows_used_host) *rows_used_host = m->ticket_U[slot];
    return 0;
}

// ---- decode_type ctc_only / ctc_att: CTC prefix beam search, and the NAT decode on the forced alignment of given labels ----
namespace cn_host {
// encoder + CTC generator with the log-posteriors of ALL rows kept in m->logits (ctc_out of the reference)
int stage_encode_ctc_rows(cn_model* m, const float* feats, int B, int T, int F, const cn_decode_opts* o, hipStream_t s) {
    CN_TRY(stage_encode(m, feats, B, T, F, o, s));
    m->ctc_maxlp_valid = true;
    return run_generator(m, m->ctc_gen, m->enc_h, B * m->Tp, m->best, m->ctc_maxlp, true, s);
}
}  // namespace cn_host

namespace {
// The common opening of cn_ctc_beam / cn_ctc_beam_ngram / cn_ctc_beam_lm (`who` in the messages): the refusals they share, encoder
// and CTC generator, the pruned labels of every frame, and the search's arguments filled.  capture_out: a capture run keeps the
// log-posteriors the search ran on (cn_fetch "ctc_out").  with_hist: the back-pointers get [B][T'][beam] scratch (the LM variant
// sizes its own once it knows its iteration count).
int ctc_search_open(cn_model* m, const std::string& who, const float* feats_dev, const float* size_ratio_dev, int B, int T, int F,
                    const cn_decode_opts* opts, int beam, int pruning, double length_penalty, const CtcBeamOut& out, bool capture_out,
                    bool with_hist, CtcBeamArgs* a, hipStream_t s) {
    // (a NAT model, or the autoregressive model with its CTC head: ArtTask decode_type 'ctc_only', src/tasks/art_task.py:252-253)
    if (!opts || m->cfg.ast == 2 || !m->ctc_gen.W || !out.hyp || !out.hyp_len || !out.score || !out.p_blk || !out.p_nblk || !out.n_out) {
        cn_set_error(who + ": needs a model with a CTC head, decode options and all output buffers");
        return -1;
    }
    if (const char* bad = cs_check_limits(beam, pruning, 0, 0)) {
        cn_set_error(who + ": " + bad);
        return -1;
    }
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(stage_encode_ctc_rows(m, feats_dev, B, T, F, opts, s));
    const int Tp = m->Tp, M = B * Tp, V = m->cfg.vocab_size;
    if (const char* bad = cs_check_limits(beam, pruning, Tp, out.Lmax)) {
        cn_set_error(who + ": " + bad);
        return -1;
    }
    if (capture_out && opts->capture) CN_TRY(capture(m, "ctc_out", m->logits, false, CN_DTYPE_F32, {B, Tp, V}, s));
    void *top_idx = nullptr, *top_val = nullptr, *hpar = nullptr, *htok = nullptr;
    const int P = pruning > 0 ? pruning : 1;  // (a zero-width pruning still needs a buffer; the kernel then sees P = 0)
    CN_TRY(scratch_buf(m, "cb_top_idx", (size_t)M * P * 4, &top_idx));
    CN_TRY(scratch_buf(m, "cb_top_val", (size_t)M * P * 4, &top_val));
    if (with_hist) {
        CN_TRY(scratch_buf(m, "cb_hist_par", (size_t)M * beam, &hpar));
        CN_TRY(scratch_buf(m, "cb_hist_tok", (size_t)M * beam * 4, &htok));
    }
    if (pruning > 0) {
        ProfScope ps(m, "ctc_topk", 0, (double)M * V * 4, s);
        CN_TRY(launch_topk(m->logits, M, V, V, pruning, (int*)top_idx, (float*)top_val, s));
    }
    *a = ctc_beam_args(m->logits, (const int*)top_idx, size_ratio_dev, B, Tp, V, beam, pruning, opts->padding_idx, length_penalty, out);
    a->hist_parent = (unsigned char*)hpar;
    a->hist_tok = (int*)htok;
    return 0;
}
// The body of cn_ctc_beam and of its n-gram, bias and merging forms (`who`; `scope`: the name in profiles): one launch of the search
// kernel (ctc_beam.hip) behind encoder, CTC head and top-k.  `a` comes with the policy (ng / lm_scale / bias / merge), size ratios,
// beam, pruning, length penalty and outputs; ctc_search_open fills the rest.  desc_missing: `who`'s own descriptor is mandatory and
// null.  What a fusing or merging search refuses is looked at before anything is launched.
int ctc_beam_call(cn_model* m, const char* who, const char* scope, bool desc_missing, CtcSearchArgs a, const float* feats_dev, int B, int T,
                  int F, const cn_decode_opts* opts, void* stream) {
    CN_TRY(check_call(m, B, T, F));
    if (a.ng && a.bias) {
        cn_set_error(std::string(who) + ": at most one of the n-gram and the bias descriptor may be set");
        return -1;
    }
    if (a.ng || a.bias || a.merge || desc_missing) {
        if (desc_missing || !a.size_ratio || !a.out.score_lm || !(a.lp == a.lp) || (a.ng && !(a.lm_scale == a.lm_scale))) {
            cn_set_error(std::string(who) + ": needs its descriptor, size ratios, length_penalty and lm_scale numbers and all output buffers");
            return -1;
        }
        const std::string bad = a.ng ? ng_check_desc(*a.ng) : a.bias ? cb_check_desc(*a.bias) : std::string();
        if (!bad.empty()) {
            cn_set_error(std::string(who) + ": " + bad);
            return -1;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    CN_TRY(ctc_search_open(m, who, feats_dev, a.size_ratio, B, T, F, opts, a.W, a.P, a.lp, a.out, true, true, &a, s));
    ProfScope ps(m, scope, 0, (double)B * a.Tp * (a.P + 1) * 4, s);
    return launch_ctc_beam(a, s);
}
// what the entries below know before the encoder has run
CtcSearchArgs ctc_call_args(const float* size_ratio_dev, int beam, int pruning, double length_penalty, const CtcBeamOut& out,
                            const cn_ngram_desc* ng = nullptr, double lm_scale = 0.0, const cn_bias_desc* bias = nullptr, bool merge = false) {
    return ctc_search_args(ctc_beam_args(nullptr, nullptr, size_ratio_dev, 0, 0, 0, beam, pruning, 0, length_penalty, out), ng, lm_scale, bias,
                           merge);
}
}  // namespace

// ctc_beam_decode (src/utils/beam_decode.py:8-93) without a language model: hyp_out_dev [B][beam][hyp_cap] labels (no sos),
// hyp_len_dev / score_dev (score_ctc, float64) / p_blk_dev / p_nblk_dev [B][beam], nbeam_dev [B] hypotheses kept (best first).
extern "C" int cn_ctc_beam(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                           const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty, int32_t* hyp_out_dev,
                           int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev, double* p_blk_dev, double* p_nblk_dev,
                           int32_t* nbeam_dev, void* stream) {
    const CtcBeamOut out = ctc_beam_out(hyp_out_dev, hyp_cap, hyp_len_dev, score_dev, nullptr, p_blk_dev, p_nblk_dev, nbeam_dev);
    return ctc_beam_call(m, "cn_ctc_beam", "ctc_prefix_beam", false, ctc_call_args(size_ratio_dev, beam, pruning, length_penalty, out),
                         feats_dev, B, T, F, opts, stream);
}

// The same search with a word n-gram model fused (ctc_ngram_search.h; not in the reference): one launch of the n-gram instantiation
// of the search kernel.  Outputs as cn_ctc_beam_lm.
extern "C" int cn_ctc_beam_ngram(cn_model* m, const cn_ngram_desc* desc, const float* feats_dev, const float* size_ratio_dev, int32_t B,
                                 int32_t T, int32_t F, const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty,
                                 double lm_scale, int32_t* hyp_out_dev, int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev,
                                 double* score_lm_dev, double* p_blk_dev, double* p_nblk_dev, int32_t* nbeam_dev, void* stream) {
    const CtcBeamOut out = ctc_beam_out(hyp_out_dev, hyp_cap, hyp_len_dev, score_dev, score_lm_dev, p_blk_dev, p_nblk_dev, nbeam_dev);
    return ctc_beam_call(m, "cn_ctc_beam_ngram", "ctc_ngram_beam", !desc,
                         ctc_call_args(size_ratio_dev, beam, pruning, length_penalty, out, desc, lm_scale), feats_dev, B, T, F, opts, stream);
}

// The same search with contextual phrase biasing (ctc_bias_search.h, include/cassnat_hip_ctc_bias.h; not in the reference): one launch
// of the bias instantiation of the search kernel.  Outputs as cn_ctc_beam_ngram.
extern "C" int cn_ctc_beam_bias(cn_model* m, const cn_bias_desc* desc, const float* feats_dev, const float* size_ratio_dev, int32_t B,
                                int32_t T, int32_t F, const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty,
                                int32_t* hyp_out_dev, int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev, double* score_lm_dev,
                                double* p_blk_dev, double* p_nblk_dev, int32_t* nbeam_dev, void* stream) {
    const CtcBeamOut out = ctc_beam_out(hyp_out_dev, hyp_cap, hyp_len_dev, score_dev, score_lm_dev, p_blk_dev, p_nblk_dev, nbeam_dev);
    return ctc_beam_call(m, "cn_ctc_beam_bias", "ctc_bias_beam", !desc,
                         ctc_call_args(size_ratio_dev, beam, pruning, length_penalty, out, nullptr, 0.0, desc), feats_dev, B, T, F, opts, stream);
}

// The same search merging candidates by prefix (ctc_merge_search.h, include/cassnat_hip_ctc_merge.h; not in the reference), without
// fusion, with the n-gram model or with the phrase list: one launch of the MERGE instantiation of that policy.  Outputs as
// cn_ctc_beam_ngram.
extern "C" int cn_ctc_beam_merged(cn_model* m, const cn_ngram_desc* ngram_desc, double lm_scale, const cn_bias_desc* bias_desc,
                                  const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                                  const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty, int32_t* hyp_out_dev,
                                  int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev, double* score_lm_dev, double* p_blk_dev,
                                  double* p_nblk_dev, int32_t* nbeam_dev, void* stream) {
    const CtcBeamOut out = ctc_beam_out(hyp_out_dev, hyp_cap, hyp_len_dev, score_dev, score_lm_dev, p_blk_dev, p_nblk_dev, nbeam_dev);
    return ctc_beam_call(m, "cn_ctc_beam_merged", "ctc_merged_beam", false,
                         ctc_call_args(size_ratio_dev, beam, pruning, length_penalty, out, ngram_desc, lm_scale, bias_desc, true), feats_dev, B,
                         T, F, opts, stream);
}

// CassNAT.beam_decode with decode_type 'ctc_att' and sample_num 1 (src/models/cassnat.py:446-448, 391-414): the trigger mask
// comes from the forced (Viterbi) alignment of the given label sequences - the best CTC beam hypotheses - instead of the greedy
// path; everything after align_to_mask is cn_decode_nast's.  labels_dev [B][ld] (no sos), label_len_dev [B].
extern "C" int cn_decode_nast_forced(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                                     const cn_decode_opts* opts, const int32_t* labels_dev, const int32_t* label_len_dev, int32_t ld,
                                     int32_t max_label_len, int32_t* hyp_out_dev, int32_t hyp_stride, int32_t* hyp_len_dev,
                                     double* score_dev, void* stream) {
    CN_TRY(check_call(m, B, T, F));
    if (!opts || m->cfg.ast || opts->beam_width < 1 || opts->beam_width > 16 || !labels_dev || !label_len_dev || max_label_len < 0 ||
        max_label_len > ld) {
        cn_set_error("cn_decode_nast_forced: bad argument");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(stage_encode_ctc_rows(m, feats_dev, B, T, F, opts, s));
    const int Tp = m->Tp, V = m->cfg.vocab_size;
    if (max_label_len > Tp) {
        cn_set_error("cn_decode_nast_forced: more labels than frames");
        return -1;
    }
    const bool cap = opts->capture != 0;
    if (cap) CN_TRY(capture(m, "ctc_out", m->logits, false, CN_DTYPE_F32, {B, Tp, V}, s));
    if (max_label_len == 0) {  // every hypothesis empty: aligned_seq_shift is all blank (cassnat.py:410-411)
        CN_TRY(launch_fill_int(m->best, (size_t)B * Tp, opts->padding_idx, s));
    } else {
        void* bp = nullptr;
        CN_TRY(scratch_buf(m, "vit_bp", (size_t)B * Tp * (2 * (size_t)max_label_len + 1), &bp));
        ViterbiArgs v;
        v.logp = m->logits;
        v.keymask = m->keymask;
        v.size_ratio = size_ratio_dev;
        v.labels = labels_dev;
        v.label_len = label_len_dev;
        v.B = B;
        v.Tp = Tp;
        v.V = V;
        v.ld = ld;
        v.ymax = max_label_len;
        v.blank = opts->padding_idx;
        v.bp = (unsigned char*)bp;
        v.out_path = m->best;
        ProfScope ps(m, "ctc_viterbi", 0, (double)B * Tp * (2 * max_label_len + 1) * 5, s);
        CN_TRY(launch_ctc_viterbi(v, s));
    }
    AlignArgs al;
    al.best = m->best;
    al.keymask = m->keymask;
    al.size_ratio = size_ratio_dev;
    al.B = B;
    al.Tp = Tp;
    al.blank = opts->padding_idx;
    al.left = opts->left_trigger;
    al.right = opts->right_trigger;
    al.shift = m->shift;
    al.src_size = m->src_size;
    al.ylen = m->ylen;
    al.ymax = m->ymax;
    al.intervals = m->intervals;
    al.raw_path = 1;
    al.ylen_in = label_len_dev;
    CN_TRY(launch_ctc_align(al, s));
    CN_HIP_CHECK(hipMemcpyAsync(m->ymax_pinned, m->ymax, sizeof(int), hipMemcpyDeviceToHost, s));
    CN_HIP_CHECK(hipStreamSynchronize(s));
    const int ymax = *m->ymax_pinned;
    if (ymax < 1 || ymax > Tp + 1 || (hyp_out_dev && hyp_stride < ymax + 1)) {
        cn_set_error("cn_decode_nast_forced: token count outside the output buffers");
        return -1;
    }
    return stage_decode(m, ymax, opts, hyp_out_dev, hyp_stride, hyp_len_dev, score_dev, s);
}

// ---- ESA: error-based sampling of alignments (src/models/cassnat.py:370-376, 441-445) ------------------------------
// cn_esa_begin runs the encoder and the CTC generator once and keeps the two best labels of every frame.  Every
// cn_esa_sample call then builds n_samples sampled alignments per utterance - in alignment g frame t of utterance b takes
// the second-best label iff its draw select[g][b][t] is 1 and the best label's probability is below `threshold` (all-zero
// draws, or select == NULL with n_samples == 1: the best path itself) - and runs the alignment + decoder side on all of
// them in ONE pass of B * n_samples query sets over the B utterances' encoder outputs (n_samples <= cfg.esa_group, which
// sizes the decoder-side workspace): tok_out / val_out [n_samples][B][out_stride] = argmax token and its log-probability per
// decoder row, ylen_out [n_samples][B] (EOS row included), *ymax_host = rows of this pass.  force_U: 0 = decode on this pass's
// own row count, > 0 = on that many rows, -1 = only count (no decode).  The random draws are the caller's (the reference takes
// them from torch.randint).
extern "C" int cn_esa_begin(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                            void* stream) {
    CN_TRY(check_call(m, B, T, F));
    if (!opts || m->cfg.ast) {
        cn_set_error("cn_esa_begin: needs a NAT model and decode options");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(stage_encode(m, feats_dev, B, T, F, opts, s));
    const int d = m->cfg.d_model, V = m->cfg.vocab_size, M = B * m->Tp;
    CN_TRY(run_linear(m, "generator_proj", m->ctc_gen, m->enc_h, d, m->logits, V, 1, M, 0, nullptr, 0, s));
    CN_TRY(launch_logsoftmax_argmax(m->logits, M, V, V, m->best, m->ctc_maxlp, 1, s));
    m->ctc_maxlp_valid = true;
    CN_TRY(launch_topk(m->logits, M, V, V, 2, m->topk_idx, m->topk_val, s));
    return 0;
}

extern "C" int cn_esa_sample(cn_model* m, const uint8_t* select_dev, int32_t n_samples, float threshold,
                             const float* size_ratio_dev, const cn_decode_opts* opts, int32_t* tok_out_dev, float* val_out_dev,
                             int32_t out_stride, int32_t* ylen_out_dev, int32_t* ymax_host, int32_t force_U, void* stream) {
    // beam_width > 1: the pass of the SELECTED alignments (src/models/cassnat.py:556-561 gathers them, :574-637 finishes with
    // top-k per row): the per-row top-k stays in the engine (cn_fetch "topk_idx" / "topk_val" / "ylen"), no token rows are copied
    const bool topk_pass = opts && opts->beam_width > 1;
    if (!m || !opts || !ymax_host || m->B < 1 || opts->beam_width < 1 || opts->beam_width > 16 ||
        (force_U >= 0 && !topk_pass && (!tok_out_dev || !val_out_dev || !ylen_out_dev))) {
        cn_set_error("cn_esa_sample: call cn_esa_begin first; 1 <= beam_width <= 16; beam_width 1 needs the output buffers");
        return -1;
    }
    if (n_samples < 1 || n_samples > std::max(1, m->cfg.esa_group) || (n_samples > 1 && !select_dev)) {
        cn_set_error("cn_esa_sample: n_samples must be in [1, cfg.esa_group] (and needs draws when > 1)");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    const int B = m->B, Tp = m->Tp, G = n_samples, BG = B * G;
    CN_TRY(launch_esa_paths(m->topk_idx, m->topk_val, select_dev, threshold, m->best, B * Tp, G, s));
    AlignArgs al;
    al.best = m->best;
    al.keymask = m->keymask;
    al.size_ratio = size_ratio_dev;
    al.B = BG;
    al.src_mod = B;  // entry g * B + b reads utterance b's mask and length
    al.Tp = Tp;
    al.blank = opts->padding_idx;
    al.left = opts->left_trigger;
    al.right = opts->right_trigger;
    al.shift = m->shift;
    al.src_size = m->src_size;
    al.ylen = m->ylen;
    al.ymax = m->ymax;
    al.intervals = m->intervals;
    CN_TRY(launch_ctc_align(al, s));
    CN_HIP_CHECK(hipMemcpyAsync(m->ymax_pinned, m->ymax, sizeof(int), hipMemcpyDeviceToHost, s));
    CN_HIP_CHECK(hipStreamSynchronize(s));
    int U = *m->ymax_pinned;
    if (force_U < 0) {  // count only: the caller wants the row count of these alignments (to take the maximum over all groups)
        *ymax_host = U;
        return 0;
    }
    if (force_U > 0) {
        // decode on force_U rows per alignment (>= this pass's own count): the conformer's GroupNorm runs over an utterance's
        // whole (channels x rows) image, padded rows included, so every group has to use the row count of ALL samples to give
        // what the reference's one big batch gives
        if (force_U < U) {
            cn_set_error("cn_esa_sample: force_U is smaller than the row count of this pass");
            return -3;
        }
        U = force_U;
    }
    if (U < 1 || U > Tp + 1 || (!topk_pass && U > out_stride)) {
        cn_set_error("cn_esa_sample: token count outside the output stride");
        return -3;
    }
    m->dec_group = G;
    const int rc = stage_decode(m, U, opts, nullptr, 0, nullptr, nullptr, s);
    m->dec_group = 1;
    if (rc) return rc;
    *ymax_host = U;
    if (topk_pass) return 0;
    CN_TRY(launch_copy_rows(tok_out_dev, out_stride, m->tok, U, U, BG, s));
    CN_TRY(launch_copy_rows(val_out_dev, out_stride, m->val, U, U, BG, s));
    CN_TRY(launch_copy_rows(ylen_out_dev, BG, m->ylen, BG, BG, 1, s));
    *ymax_host = U;
    return 0;
}

// ---- TransformerLM scoring (src/models/lm.py:52-56 as used at cassnat.py:507-523): score[b][u] = log p(tgt[b][u] | tok[b][..u])
// under the causal + length mask (key j allowed iff j <= u and j < len[b]).  Model created with cfg.ast == 2:
// n_enc encoder layers of width d_encff, parameters text_embed.0.lut / encoder.* / out_generator.proj.
extern "C" int cn_lm_score(cn_model* m, const int32_t* tok_dev, const int32_t* tgt_dev, const int32_t* len_dev, int32_t B,
                           int32_t U, int32_t ld, float* score_dev, void* stream) {
    if (!m || m->cfg.ast != 2 || !m->finalized || !m->tgt_lut) {
        cn_set_error("cn_lm_score: the model was not created with cfg.ast = 2 / not finalized");
        return -1;
    }
    if (B < 1 || U < 1 || ld < U || (size_t)B * U > (size_t)m->maxB * (m->maxTp + 1) || U > m->pe_rows) {
        cn_set_error("cn_lm_score: batch x length exceeds the workspace");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(build_workspace(m));
    const int d = m->cfg.d_model, V = m->cfg.vocab_size, M = B * U;
    float* x = m->x;
    CN_TRY(launch_lm_embed(tok_dev, ld, m->tgt_lut, m->pe, x, B, U, d, sqrtf((float)d), s));
    static const bool no_chain = cn_exp_env("CASSNAT_NO_CHAIN") != nullptr;
    if (!m->enc.empty() && m->enc_chain.size() == m->enc.size() && !no_chain) {
        // bf16 / d_model 256: per layer [causal + length-masked attention] + one row-chain launch, as in stage_encode
        if (m->enc_entry.w) {
            CN_TRY(run_chain(m, m->enc_entry, x, M, m->qkv, 3 * d, true, CHX_NO_STORE, s));
        } else {
            CN_TRY(run_ln(m, m->enc[0].n[0], x, m->xn, M, s));
            CN_TRY(run_linear(m, "qkv_proj", m->enc[0].qkv, m->xn, d, m->qkv, 3 * d, 0, M, 0, nullptr, 0, s));
        }
        for (size_t n = 0; n < m->enc.size(); ++n) {
            const bool last = n + 1 == m->enc.size();
            CN_TRY(run_self_attn_core(m, B, U, nullptr, len_dev, 1, s));
            const int xm = (n > 0 ? CHX_IN_BLK : 0) | (last ? CHX_NO_STORE : CHX_OUT_BLK);
            CN_TRY(run_chain(m, m->enc_chain[n], x, M, last ? m->enc_h : m->qkv, last ? d : 3 * d, true, xm, s));
        }
    } else {
        for (size_t n = 0; n < m->enc.size(); ++n) {
            const Layer& L = m->enc[n];
            CN_TRY(run_self_attn(m, L, &L.n[0], x, B, U, nullptr, len_dev, 1, s));
            CN_TRY(run_ffn(m, L, L.n[1], x, M, nullptr, nullptr, s));
        }
        CN_TRY(run_ln(m, m->enc_norm, x, m->enc_h, M, s));
    }
    static const bool no_fused = cn_exp_env("CASSNAT_LM_NO_FUSED_TAIL") != nullptr;
    if (m->att_gen.gm_w && !no_fused) {  // bf16 / d_model 256: generator + log-softmax + gather in one kernel, no (M, V) tensor
        const bool x3 = m->prec == CN_PREC_X3;
        ProfScope ps(m, "generator_gather_fused", (x3 ? 6.0 : 2.0) * M * V * d, ((double)M * d + (double)V * d) * (x3 ? 4 : 2), s);
        GenmaxArgs a;
        a.x3 = x3;
        a.h = m->enc_h;
        a.wp = m->att_gen.gm_w;
        a.bp = m->att_gen.gm_b;
        a.M = M;
        a.V = V;
        a.d = d;
        a.tgt = tgt_dev;
        a.tgt_lp = score_dev;
        a.tgt_U = U;
        a.tgt_ld = ld;
        return launch_genmax(a, s);
    }
    CN_TRY(run_linear(m, "generator_proj", m->att_gen, m->enc_h, d, m->logits, V, 1, M, 0, nullptr, 0, s));
    CN_TRY(launch_logsoftmax_argmax(m->logits, M, V, V, m->best, m->ctc_maxlp, 1, s));
    m->ctc_maxlp_valid = true;
    return launch_gather_logp(m->logits, V, tgt_dev, ld, score_dev, B, U, s);
}

// ---- CASS-NAT + LM: the finish loop of CassNAT.beam_decode with args.lm_weight > 0 (src/models/cassnat.py:574-637) ------------
// src/tasks/cassnat_task.py:85-127 + cassnat.py:603-607: the TransformerLM whose step the finish loop fuses (NULL detaches).
extern "C" int cn_nat_attach_lm(cn_model* m, cn_model* lm) {
    if (!m || m->cfg.ast != 0) {
        cn_set_error("cn_nat_attach_lm: the first handle must be a CASS-NAT model (cfg.ast = 0)");
        return -1;
    }
    if (!lm) {
        m->ast_lm = nullptr;
        return 0;
    }
    if (m->ast_ng_on) {
        cn_set_error("cn_nat_attach_lm: an n-gram model is attached (cn_nat_attach_ngram); it and a TransformerLM cannot be fused together");
        return -1;
    }
    CN_TRY(lm_check_pair(m, lm, "cn_nat_attach_lm"));
    m->ast_lm = lm;
    return 0;
}

// ymax steps of [LM step on every slot -> fused row top-k -> beam update]; the step count and every utterance's last step are
// known before the loop starts, so nothing is read back inside it.
extern "C" int cn_nat_lm_finish(cn_model* m, const cn_decode_opts* opts, int32_t ymax, int32_t beam_width, float lm_weight,
                                int32_t use_length_penalty, double length_penalty, int32_t zero_past_len, int32_t* hyp_out_dev,
                                int32_t max_len, int32_t* hyp_len_dev, double* score_dev, void* stream) {
    if (!m || !opts || !hyp_out_dev || !hyp_len_dev || !score_dev) {
        cn_set_error("cn_nat_lm_finish: null argument");
        return -1;
    }
    cn_model* lm = m->ast_lm;
    if (m->cfg.ast != 0 || !lm || !(lm_weight > 0.f)) {
        cn_set_error("cn_nat_lm_finish: needs lm_weight > 0 and an LM attached with cn_nat_attach_lm");
        return -1;
    }
    const int bw = beam_width, B = m->B, U = m->att_rows_U, V = m->cfg.vocab_size, L = max_len;
    if (U < 1 || B < 1) {
        cn_set_error("cn_nat_lm_finish: the last decode pass kept no log-probability rows (set cn_decode_opts.reserved[0], one "
                     "alignment per utterance)");
        return -1;
    }
    if (bw < 1 || bw > 16 || bw > V || ymax < 1 || ymax > U || L < ymax + 1) {
        cn_set_error("cn_nat_lm_finish: need 1 <= beam_width <= 16, 1 <= ymax <= rows of the pass and max_len >= ymax + 1");
        return -1;
    }
    const int S = B * bw;
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(lm_check_step(lm, L, S, "cn_nat_lm_finish"));
    CN_TRY(lm_prepare_buffers(lm, L, S));
    NatBeamState st;
    void* p = nullptr;
    for (int i = 0; i < 2; ++i) {
        CN_TRY(scratch_buf(m, i ? "nat_tok1" : "nat_tok0", (size_t)S * L * 4, &p));
        st.tok[i] = (int*)p;
        CN_TRY(scratch_buf(m, i ? "nat_anc1" : "nat_anc0", (size_t)S * L * 4, &p));
        st.anc[i] = (int*)p;
        CN_TRY(scratch_buf(m, i ? "nat_keyok1" : "nat_keyok0", (size_t)S * L, &p));
        st.keyok[i] = (unsigned char*)p;
        CN_TRY(scratch_buf(m, i ? "nat_score1" : "nat_score0", (size_t)S * 8, &p));
        st.score[i] = (double*)p;
    }
    CN_TRY(scratch_buf(m, "nat_cur_tok", (size_t)S * 4, &p));
    st.cur_tok = (int*)p;
    int *last = nullptr, *cidx = nullptr;
    float* cval = nullptr;
    CN_TRY(scratch_buf(m, "nat_last", (size_t)B * 4, (void**)&last));
    CN_TRY(scratch_buf(m, "nat_cand_idx", (size_t)S * bw * 4, (void**)&cidx));
    CN_TRY(scratch_buf(m, "nat_cand_val", (size_t)S * bw * 4, (void**)&cval));
    CN_TRY(launch_nat_beam_init(st, m->ylen, ymax, last, hyp_len_dev, B, bw, L, opts->sos, opts->padding_idx, s));
    int cur = 0;
    for (int step = 0; step < ymax; ++step) {
        CN_TRY(lm_step_run(lm, S, step, st.cur_tok, st.anc[cur], st.keyok[cur], L, s));
        NatFuseArgs f;
        f.att = m->logits;
        f.lm = lm->ast_logits;
        f.last = last;
        f.zlen = zero_past_len ? m->ylen : nullptr;
        f.idx = cidx;
        f.val = cval;
        f.U = U;
        f.V = V;
        f.bw = bw;
        f.step = step;
        f.k = bw;
        f.w = lm_weight;
        {
            ProfScope ps(m, "nat_lm_fuse_topk", 0, 2.0 * S * V * 4, s);
            CN_TRY(launch_nat_lm_fuse_topk(f, S, s));
        }
        NatBeamStep q;
        q.idx = cidx;
        q.val = cval;
        q.last = last;
        q.cur = cur;
        q.step = step;
        q.bw = bw;
        q.L = L;
        q.pad = opts->padding_idx;
        q.use_lp = use_length_penalty;
        q.lp = length_penalty;
        CN_TRY(launch_nat_beam_update(st, q, B, s));
        cur ^= 1;
    }
    CN_HIP_CHECK(hipMemcpyAsync(hyp_out_dev, st.tok[cur], (size_t)S * L * 4, hipMemcpyDeviceToDevice, s));
    CN_HIP_CHECK(hipMemcpyAsync(score_dev, st.score[cur], (size_t)S * 8, hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---- CTC prefix beam search with the TransformerLM in the frame loop (src/utils/beam_decode.py:8-93, args.ctc_lm_weight > 0) ----
// One iteration per processed frame: [LM step on every slot, a position per row -> log-softmax -> LM rows of the beam -> frame
// step]; which frames an utterance processes is known from ctc_out, so the host reads the iteration count once and nothing
// returns inside the loop (kernels and cache addressing: ctc_lm.hip).  Outputs as cn_ctc_beam plus score_lm_dev [B][beam].
extern "C" int cn_ctc_beam_lm(cn_model* m, cn_model* lm, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T,
                              int32_t F, const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty,
                              double lm_weight, int32_t* hyp_out_dev, int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev,
                              double* score_lm_dev, double* p_blk_dev, double* p_nblk_dev, int32_t* nbeam_dev, int32_t* iterations_host,
                              void* stream) {
    CN_TRY(check_call(m, B, T, F));
    if (!opts || !score_lm_dev) {
        cn_set_error("cn_ctc_beam_lm: needs decode options and all output buffers");
        return -1;
    }
    CN_TRY(lm_check_pair(m, lm, "cn_ctc_beam_lm"));
    const int V = m->cfg.vocab_size, blank = opts->padding_idx, sos = opts->sos;
    if (!(lm_weight == lm_weight) || blank < 0 || blank >= V || sos < 0 || sos >= V || sos == blank) {
        cn_set_error("cn_ctc_beam_lm: lm_weight must be a number; blank and sos two different ids of the vocabulary");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const CtcBeamOut o = ctc_beam_out(hyp_out_dev, hyp_cap, hyp_len_dev, score_dev, score_lm_dev, p_blk_dev, p_nblk_dev, nbeam_dev);
    CtcLmFrame a;
    CN_TRY(ctc_search_open(m, "cn_ctc_beam_lm", feats_dev, size_ratio_dev, B, T, F, opts, beam, pruning, length_penalty, o, true, false, &a, s));
    const int Tp = a.Tp, M = B * Tp, W = beam, S = B * W;
    void* p = nullptr;
    int *frames = nullptr, *count = nullptr;
    CN_TRY(scratch_buf(m, "cl_frames", (size_t)M * 4, (void**)&frames));
    CN_TRY(scratch_buf(m, "cl_count", (size_t)B * 4, (void**)&count));
    CN_TRY(launch_ctc_lm_schedule(m->logits, size_ratio_dev, B, Tp, V, blank, frames, count, s));
    // the one host read: the iteration count (the passes sync once for their row count too)
    std::vector<int> hcount(B);
    CN_HIP_CHECK(hipMemcpyAsync(hcount.data(), count, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    CN_HIP_CHECK(hipStreamSynchronize(s));
    const int K = *std::max_element(hcount.begin(), hcount.end());
    if (iterations_host) *iterations_host = K;
    // a hypothesis gains at most one label per iteration: prefixes reach K + 1 tokens, LM positions K; K * S cache rows per layer
    const int Lt = K + 2;
    if (lm_check_step(lm, K + 1, S, "cn_ctc_beam_lm") != 0) {
        cn_set_error("cn_ctc_beam_lm: the LM handle is too small: " + std::to_string(S) + " beam slots (B x ctc_beam) need max_batch x "
                     "(max_frames / 4 + 1) >= " + std::to_string(S) + " (have " + std::to_string((size_t)lm->maxB * (lm->maxTp + 1)) +
                     "), " + std::to_string(K) + " processed frames need a position table of " + std::to_string(K + 1) + " rows (have " +
                     std::to_string(lm->pe_rows) + ")");
        return -1;
    }
    CN_TRY(lm_prepare_buffers(lm, K + 1, S));
    CtcLmState st;
    CN_TRY(scratch_buf(m, "cl_pb", (size_t)S * 8, &p));
    st.pb = (double*)p;
    CN_TRY(scratch_buf(m, "cl_pnb", (size_t)S * 8, &p));
    st.pnb = (double*)p;
    CN_TRY(scratch_buf(m, "cl_sctc", (size_t)S * 8, &p));
    st.sctc = (double*)p;
    CN_TRY(scratch_buf(m, "cl_slm", (size_t)S * 8, &p));
    st.slm = (double*)p;
    int** ints[] = {&st.len, &st.last, &st.tok, &st.pos, &st.parent, &st.stay};
    const char* names[] = {"cl_len", "cl_last", "cl_tok", "cl_pos", "cl_parent", "cl_stay"};
    for (int i = 0; i < 6; ++i) {
        CN_TRY(scratch_buf(m, names[i], (size_t)S * 4, &p));
        *ints[i] = (int*)p;
    }
    CN_TRY(scratch_buf(m, "cl_nb", (size_t)B * 4, &p));
    st.nb = (int*)p;
    float* lmrow[2];
    for (int i = 0; i < 2; ++i) {
        CN_TRY(scratch_buf(m, i ? "cl_rowid1" : "cl_rowid0", (size_t)S * Lt * 4, &p));
        st.rowid[i] = (int*)p;
        CN_TRY(scratch_buf(m, i ? "cl_lmrow1" : "cl_lmrow0", (size_t)S * V * 4, &p));
        lmrow[i] = (float*)p;
        CN_HIP_CHECK(hipMemsetAsync(p, 0, (size_t)S * V * 4, s));  // (an unused slot copies its own row: never uninitialised memory)
    }
    const int hs = K > 0 ? K : 1;
    void *hpar = nullptr, *htok = nullptr;
    CN_TRY(scratch_buf(m, "cl_hist_par", (size_t)B * hs * W, &hpar));
    CN_TRY(scratch_buf(m, "cl_hist_tok", (size_t)B * hs * W * 4, &htok));
    CN_TRY(launch_ctc_lm_init(st, B, W, Lt, sos, s));
    a.frames = frames, a.count = count, a.hist_parent = (unsigned char*)hpar, a.hist_tok = (int*)htok;
    a.sos = sos, a.Lt = Lt, a.hist_stride = hs, a.lm_weight = lm_weight;
    for (int k = 0; k < K; ++k) {
        CN_TRY(lm_step_run(lm, S, k, st.tok, st.rowid[k & 1], nullptr, Lt, s, st.pos, st.stay));
        CN_TRY(launch_logsoftmax_argmax(lm->ast_logits, S, V, V, lm->best, lm->ctc_maxlp, 1, s));
        {
            ProfScope ps(m, "ctc_lm_rows", 0, 2.0 * S * V * 4, s);
            CN_TRY(launch_ctc_lm_rows(lm->ast_logits, lmrow[(k & 1) ^ 1], lmrow[k & 1], st.parent, st.stay, count, k, S, W, V, s));
        }
        a.lmrow = lmrow[k & 1];
        a.iter = k;
        ProfScope ps(m, "ctc_lm_frame", 0, (double)S * (pruning + 1) * 8, s);
        CN_TRY(launch_ctc_lm_frame(st, a, s));
    }
    return launch_ctc_lm_finish(st, o, count, (const unsigned char*)hpar, (const int*)htok, hs, B, W, s);
}

