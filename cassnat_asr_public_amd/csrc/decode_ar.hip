// The autoregressive decoder (cfg.ast = 1) and the TransformerLM step (cfg.ast = 2): their step caches, one decoding step of
// either, and the entries cn_ast_*, cn_lm_step* and cn_decode_ast (the beam search on the device).
#include <algorithm>
#include <cmath>

#include "ast_bias_search.h"
#include "ast_ngram_search.h"
#include "model.h"

using namespace cn_host;

// ESA ranking with rank_model == 'at_baseline' (src/models/cassnat.py:514-520; Transformer.forward_decoder,
// src/models/transformer.py:113-116): the autoregressive model (cfg.ast = 1) scores the NAT predictions teacher-forced.
// Its own encoder runs on the B utterances; the decoder then takes N = B * n_per_utt token rows (row e belongs to utterance
// e % B: the sample-major order of cn_esa_sample) under the causal + length mask, with cross attention to its utterance's
// encoder output under the padding mask: score[e][u] = log softmax(att_generator(dec_h))[e][u][tgt[e][u]] (the reference
// takes the probability itself: exp on the caller's side).  tok / tgt / score are [N][ld], ld >= U; cfg.esa_group >= n_per_utt.
extern "C" int cn_ast_teacher_score(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                                    const int32_t* tok_dev, const int32_t* tgt_dev, const int32_t* len_dev, int32_t n_per_utt,
                                    int32_t U, int32_t ld, float* score_dev, void* stream) {
    CN_TRY(check_call(m, B, T, F));
    if (!opts || m->cfg.ast != 1 || !m->tgt_lut || n_per_utt < 1 || n_per_utt > std::max(1, m->cfg.esa_group) || U < 1 || ld < U ||
        U > m->pe_rows) {
        cn_set_error("cn_ast_teacher_score: needs an autoregressive model (cfg.ast = 1) whose cfg.esa_group covers the samples per utterance");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(stage_encode(m, feats_dev, B, T, F, opts, s));
    const int d = m->cfg.d_model, V = m->cfg.vocab_size, Tp = m->Tp, N = B * n_per_utt, M = N * U;
    if ((size_t)M > (size_t)m->maxB * (m->maxTp + 1) * std::max(1, m->cfg.esa_group)) {
        cn_set_error("cn_ast_teacher_score: token rows exceed the workspace");
        return -1;
    }
    m->dec_group = n_per_utt;  // N query sets over the B utterances' encoder outputs
    float* x = m->xd;
    CN_TRY(launch_lm_embed(tok_dev, ld, m->tgt_lut, m->pe, x, N, U, d, sqrtf((float)d), s));
    for (size_t i = 0; i < m->mad.size(); ++i) {  // DecoderLayer: self attention, source attention, feed-forward
        const Layer& L = m->mad[i];
        CN_TRY(run_self_attn(m, L, &L.n[0], x, N, U, nullptr, len_dev, 1, s));
        CN_TRY(run_src_attn(m, L, &L.n[1], x, N, U, Tp, nullptr, s));
        CN_TRY(run_ffn(m, L, L.n[2], x, M, nullptr, nullptr, s));
    }
    CN_TRY(run_ln(m, m->dec_norm, x, m->dec_h, M, s));
    // generator in chunks of whole token rows that fit the logits buffer (B * (T' + 1) rows)
    const int cap_rows = m->maxB * (m->maxTp + 1);
    const int seq_per = std::max(1, cap_rows / U);
    for (int e0 = 0; e0 < N; e0 += seq_per) {
        const int ne = std::min(seq_per, N - e0), rows = ne * U;
        const void* h = (const unsigned char*)m->dec_h + (size_t)e0 * U * d * m->es;
        CN_TRY(run_linear(m, "generator_proj", m->att_gen, h, d, m->logits, V, 1, rows, 0, nullptr, 0, s));
        CN_TRY(launch_logsoftmax_argmax(m->logits, rows, V, V, m->tok, m->val, 1, s));
        CN_TRY(launch_gather_logp(m->logits, V, tgt_dev + (size_t)e0 * ld, ld, score_dev + (size_t)e0 * ld, ne, U, s));
    }
    m->dec_group = 1;
    return 0;
}

// ArtTask decode_type 'ctc_correct' (Transformer.fast_decode_with_ctc, src/models/transformer.py:243-342): the CTC greedy hypothesis
// of every utterance, behind sos, is the decoder's teacher-forced input under the causal + padding mask; the finish loop then reads
// the k best labels of row i while i <= length[b].  Device part: encoder, CTC arg-max + collapse, decoder, generator + log-softmax +
// top-k.  Outputs: len_out_dev [B] (CTC labels per utterance), tok_out_dev / val_out_dev [B][U][k] (U = longest + 1 rows, returned
// in *rows_host; the buffers hold B * (T' + 1) * k entries).  One host sync on the longest hypothesis (the reference's max(length)).
extern "C" int cn_ast_ctc_correct(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                                  int32_t k, int32_t* tok_out_dev, float* val_out_dev, int32_t* len_out_dev, int32_t* rows_host,
                                  void* stream) {
    CN_TRY(check_call(m, B, T, F));
    if (!opts || m->cfg.ast != 1 || !m->tgt_lut || !m->ctc_gen.W || k < 1 || k > 16 || !tok_out_dev || !val_out_dev || !len_out_dev ||
        !rows_host) {
        cn_set_error("cn_ast_ctc_correct: needs an autoregressive model (cfg.ast = 1) with a CTC head, 1 <= k <= 16 and all output buffers");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(stage_encode_ctc_rows(m, feats_dev, B, T, F, opts, s));
    const int d = m->cfg.d_model, V = m->cfg.vocab_size, Tp = m->Tp, ld = Tp + 1;
    if (ld > m->pe_rows) {
        cn_set_error("cn_ast_ctc_correct: more subsampled frames than rows of the positional table");
        return -1;
    }
    void *tgt = nullptr, *keylen = nullptr;
    CN_TRY(scratch_buf(m, "cc_tgt", (size_t)B * ld * 4, &tgt));
    CN_TRY(scratch_buf(m, "cc_keylen", (size_t)B * 4, &keylen));
    CN_TRY(launch_ctc_collapse(m->best, m->keymask, B, Tp, opts->sos, opts->padding_idx, ld, (int*)tgt, len_out_dev, (int*)keylen, m->ymax, s));
    CN_HIP_CHECK(hipMemcpyAsync(m->ymax_pinned, m->ymax, sizeof(int), hipMemcpyDeviceToHost, s));
    CN_HIP_CHECK(hipStreamSynchronize(s));  // the decoder's row count is data dependent (max_length + 1, transformer.py:266)
    const int U = *m->ymax_pinned + 1, M = B * U;
    if (U < 1 || U > ld) {
        cn_set_error("cn_ast_ctc_correct: impossible CTC hypothesis length");
        return -3;
    }
    m->dec_group = 1;
    float* x = m->xd;
    CN_TRY(launch_lm_embed((const int*)tgt, ld, m->tgt_lut, m->pe, x, B, U, d, sqrtf((float)d), s));
    for (size_t i = 0; i < m->mad.size(); ++i) {  // DecoderLayer: self attention (causal + padding mask), source attention, feed-forward
        const Layer& L = m->mad[i];
        CN_TRY(run_self_attn(m, L, &L.n[0], x, B, U, nullptr, (const int*)keylen, 1, s));
        CN_TRY(run_src_attn(m, L, &L.n[1], x, B, U, Tp, nullptr, s));
        CN_TRY(run_ffn(m, L, L.n[2], x, M, nullptr, nullptr, s));
    }
    CN_TRY(run_ln(m, m->dec_norm, x, m->dec_h, M, s));
    CN_TRY(run_linear(m, "generator_proj", m->att_gen, m->dec_h, d, m->logits, V, 1, M, 0, nullptr, 0, s));
    CN_TRY(launch_logsoftmax_argmax(m->logits, M, V, V, m->tok, m->val, 1, s));
    CN_TRY(launch_topk(m->logits, M, V, V, k, tok_out_dev, val_out_dev, s));
    *rows_host = U;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// AST (autoregressive) path: BASELINE config 4
// ---------------------------------------------------------------------------------------------------------------------
namespace cn_host {
namespace {
int ast_alloc(cn_model* m, void** p, size_t bytes) {
    CN_HIP_CHECK(hipMalloc(p, bytes ? bytes : 256));
    m->ast_allocs.push_back(*p);
    return 0;
}

int ast_prepare_buffers(cn_model* m, int max_len, int max_slots, int ctc_beam) {
    if (m->ast_max_len >= max_len && m->ast_slots >= max_slots && m->ast_ctc_beam >= ctc_beam && m->ast_Tp_cap >= m->maxTp)
        return 0;
    for (void* q : m->ast_allocs) (void)hipFree(q);
    m->ast_allocs.clear();
    m->beam_S = m->beam_L = m->beam_K = 0;  // the beam-search state lives in the same allocation list
    m->ast_kvx.clear();
    m->ast_ck.clear();
    m->ast_cv.clear();
    const size_t d = m->cfg.d_model, V = m->cfg.vocab_size, es = m->es;
    const size_t Mmem = (size_t)m->maxB * m->maxTp;
    for (size_t l = 0; l < m->mad.size(); ++l) {
        void *kvx = nullptr, *ck = nullptr, *cv = nullptr;
        CN_TRY(ast_alloc(m, &kvx, Mmem * 2 * d * es));
        CN_TRY(ast_alloc(m, &ck, (size_t)max_len * max_slots * d * es));
        CN_TRY(ast_alloc(m, &cv, (size_t)max_len * max_slots * d * es));
        m->ast_kvx.push_back(kvx);
        m->ast_ck.push_back(ck);
        m->ast_cv.push_back(cv);
    }
    CN_TRY(ast_alloc(m, (void**)&m->ast_logits, (size_t)max_slots * V * 4));
    CN_TRY(ast_alloc(m, (void**)&m->ast_arg, (size_t)max_slots * 4));
    CN_TRY(ast_alloc(m, (void**)&m->ast_maxlp, (size_t)max_slots * 4));
    CN_TRY(ast_alloc(m, (void**)&m->ast_r0, Mmem * 2 * 4));
    const int kb = ctc_beam > 0 ? ctc_beam : 1;
    for (int i = 0; i < 2; ++i) CN_TRY(ast_alloc(m, (void**)&m->ast_r[i], (size_t)max_slots * kb * m->maxTp * 2 * 4));
    m->ast_max_len = max_len;
    m->ast_slots = max_slots;
    m->ast_ctc_beam = ctc_beam;
    m->ast_Tp_cap = m->maxTp;
    return 0;
}
}  // namespace

// is this LM handle usable beside model m (an attach, or a call that takes both handles)?
int lm_check_pair(const cn_model* m, const cn_model* lm, const char* who) {
    if (!lm || lm->cfg.ast != 2 || !lm->finalized) {
        cn_set_error(std::string(who) + ": the LM handle must be a finalized TransformerLM (cfg.ast = 2)");
        return -1;
    }
    if (lm->lib_tag != m->lib_tag) {
        cn_set_error(std::string(who) + ": the two handles come from different libraries");
        return -1;
    }
    if (lm->cfg.vocab_size != m->cfg.vocab_size || lm->cfg.device != m->cfg.device) {
        cn_set_error(std::string(who) + ": the LM must have the model's vocabulary and device");
        return -1;
    }
    return 0;
}

// the range of one step of handle m (decoder or LM) against its step cache and tables; K = 0: the entry takes no top-K
int step_check(const cn_model* m, const char* who, int n, int pos, int table_stride, int K) {
    if (n < 1 || n > m->ast_slots || pos < 0 || pos >= m->ast_max_len || pos >= m->pe_rows || table_stride <= pos ||
        (K != 0 && (K < 1 || K > 32 || K > m->cfg.vocab_size))) {
        cn_set_error(std::string(who) + ": rows / position / K outside the configured cache (1 <= rows <= slots, 0 <= position < max_len, "
                     "the position table and table_stride; 1 <= K <= 32 and <= the vocabulary)");
        return -1;
    }
    return 0;
}

// the TransformerLM's step cache [layer][pos][slot][d] (K and V) and its logits [slot][V], on the LM handle
int lm_prepare_buffers(cn_model* lm, int max_len, int max_slots) {
    CN_TRY(build_workspace(lm));
    if (lm->ast_max_len >= max_len && lm->ast_slots >= max_slots) return 0;
    for (void* q : lm->ast_allocs) (void)hipFree(q);
    lm->ast_allocs.clear();
    lm->ast_ck.clear();
    lm->ast_cv.clear();
    const size_t d = lm->cfg.d_model, V = lm->cfg.vocab_size, es = lm->es;
    for (size_t l = 0; l < lm->enc.size(); ++l) {
        void *ck = nullptr, *cv = nullptr;
        CN_TRY(ast_alloc(lm, &ck, (size_t)max_len * max_slots * d * es));
        CN_TRY(ast_alloc(lm, &cv, (size_t)max_len * max_slots * d * es));
        lm->ast_ck.push_back(ck);
        lm->ast_cv.push_back(cv);
    }
    CN_TRY(ast_alloc(lm, (void**)&lm->ast_logits, (size_t)max_slots * V * 4));
    lm->ast_max_len = max_len;
    lm->ast_slots = max_slots;
    return 0;
}

int lm_check_step(const cn_model* lm, int max_len, int max_slots, const char* who) {
    if (!lm || lm->cfg.ast != 2 || !lm->finalized || !lm->tgt_lut) {
        cn_set_error(std::string(who) + ": the LM must be a finalized TransformerLM handle (cfg.ast = 2)");
        return -1;
    }
    if ((size_t)max_slots > (size_t)lm->maxB * (lm->maxTp + 1) || max_len > lm->pe_rows) {
        cn_set_error(std::string(who) + ": the LM handle's workspace (max_batch x max_frames) or position table is too small for "
                     "the beam's slots / max_len");
        return -1;
    }
    return 0;
}

namespace {
// The rows of one decoding step: the newest position of n hypotheses (already embedded into the stack's stream), each with the
// tables its cache attention gathers through.
struct StepRows {
    int n = 0, pos = 0;                // rows; the step's position (with row_pos: the largest of them)
    const int32_t* anc = nullptr;      // [n][table_stride] cache slot that wrote every prefix position (with row_pos: cache ROW ids)
    const uint8_t* keyok = nullptr;    // [n][table_stride] key allowed (unused with row_pos: every key is)
    int table_stride = 0;
    const int32_t* row_pos = nullptr;  // a position per row (the CTC prefix beam, whose hypotheses differ in length) ...
    const int32_t* row_stay = nullptr; // ... and the rows that append nothing (their output is garbage the caller discards)
    const int32_t* utt = nullptr;      // [n] utterance of the row: whose memory a layer's source attention reads
    int dense_bw = 0;                  // > 0: the rows are the dense slots b * dense_bw + j of the device beam (utt[row] = row / dense_bw)
};
// A stack of pre-norm layers whose self-attention reads the step cache m->ast_ck / ast_cv: the decoder's (m->mad, with source
// attention over m->ast_kvx) or the TransformerLM's (m->enc).
struct StepStack {
    const std::vector<Layer>& layers;
    int ffn_norm;            // the Layer::n[] that precedes the feed-forward sublayer
    const Norm& final_norm;  // behind the last layer, into ...
    void* final_out;
    float* x;                // the residual stream [n][d]
    const char *tag_qkv, *tag_attn, *tag_attn_rows, *tag_out, *tag_ffn_split;  // ProfScope tags
};

// x += FFN(LN x) on the n rows of a step.  A decode step has few rows (live hypotheses, <= batch x beam): the fused feed-forward
// kernel would put them on ceil(n / 64) workgroups that each stream the whole 2 MB of W1|W2.  Its d_ff split spreads the hidden
// units over 8 workgroups per row tile; the reduce kernel that adds the slices also writes the LayerNorm the next sublayer
// starts with into next_out, and *have_next says so (otherwise: the plain sublayer, nothing behind it).  Only where the layer
// has the fused kernel's streams, while the rows are few, and the slices fit the hidden-activation buffer they borrow.
// (L.w1.N is the stack's d_encff / d_decff in every layer: weights.hip packs each layer of a stack with that one width.)
int run_ffn_step(cn_model* m, const Layer& L, const Norm& norm, float* x, int n, const Norm& next_norm, void* next_out,
                 const char* tag, hipStream_t s, bool* have_next) {
    static const bool no_split = cn_exp_env("CASSNAT_AST_NO_FFN_SPLIT") != nullptr;
    const cn_config& c = m->cfg;
    const int d = c.d_model, dff = L.w1.N;
    const int ffn_slices = (!L.w1p || no_split) ? 1 : (dff % (128 * 8) == 0 ? 8 : (dff % (128 * 4) == 0 ? 4 : 1));
    const size_t hbuf_bytes = (size_t)m->maxB * (m->maxTp + 1) * std::max(1, c.esa_group) *
                              (size_t)std::max(std::max(c.d_encff, c.d_decff), c.d_ff) * m->es;
    const bool split_now = ffn_slices > 1 && n <= 2048 && (size_t)ffn_slices * n * d * 4 <= hbuf_bytes;
    *have_next = split_now;
    if (!split_now) return run_ffn(m, L, norm, x, n, nullptr, nullptr, s);
    ProfScope ps(m, tag, 4.0 * n * (double)dff * d, 2.0 * dff * d * 2 + (double)n * d * (8 + 4 * ffn_slices), s);
    FfnFusedArgs f;
    f.x = x;
    f.ln_a = norm.a;
    f.ln_b = norm.b;
    f.w1p = L.w1p;
    f.b1 = L.w1.b;
    f.w2p = L.w2p;
    f.b2 = L.w2.b;
    f.M = n;
    f.d = d;
    f.dff = dff;
    f.nslice = ffn_slices;
    f.partial = reinterpret_cast<float*>(m->hbuf);  // [slices][n][256] fp32 <= the [rows][d_ff] hidden buffer
    f.act = L.ff_swish ? FF_ACT_SWISH : FF_ACT_RELU;
    CN_TRY(launch_ffn_fused(f, s));
    return launch_ffn_reduce(x, f.partial, ffn_slices, L.w2.b, next_norm.a, next_norm.b, next_out, n, 1e-6f, s);
}

// x += O(SrcAttn(LN x, memory)) of decoder layer l on the rows of a step: the memory's K | V are m->ast_kvx[l] (cn_ast_begin)
int run_src_attn_step(cn_model* m, const Layer& L, size_t l, float* x, const StepRows& r, float scale, hipStream_t s) {
    const int d = m->cfg.d_model, H = m->cfg.n_head, n = r.n;
    CN_TRY(run_ln(m, L.n[1], x, m->xn, n, s));
    CN_TRY(run_linear(m, "src_q_proj", L.src_q, m->xn, d, m->qd, d, 0, n, 0, nullptr, 0, s));
    static const bool no_fast_src = cn_exp_env("CASSNAT_AST_GATHER_SRC") != nullptr;
    if (m->prec == CN_PREC_BF16 && m->Tp <= 256 && !no_fast_src) {
        // every hypothesis row is a batch entry of one query whose keys / values are its utterance's: the LDS-resident
        // attention kernel (K|V of a (row, head) by LDS-DMA, MFMA products) instead of the scalar gather kernel
        ProfScope ps(m, "ast_src_attention", 4.0 * n * H * m->Tp * 64, 2.0 * n * m->Tp * d * m->es, s);
        AttnArgs a2;
        a2.Q = m->qd;
        a2.K = m->ast_kvx[l];
        a2.V = (const unsigned char*)m->ast_kvx[l] + (size_t)d * m->es;
        a2.O = m->ctx;
        a2.ldq = d;
        a2.ldk = a2.ldv = 2 * d;
        a2.ldo = d;
        a2.H = H;
        a2.Lk = m->Tp;
        a2.keymask = m->keymask;
        if (r.dense_bw > 0 && n % r.dense_bw == 0) {  // device beam: utterance b owns rows b * bw .. + bw - 1
            a2.B = n / r.dense_bw;
            a2.Lq = r.dense_bw;
        } else {  // caller-managed rows: every row is a batch entry of one query that names its utterance
            a2.B = n;
            a2.Lq = 1;
            a2.kv_index = r.utt;
        }
        a2.scale = scale;
        CN_TRY(launch_attention(m->prec, a2, s));
    } else {
        GatherAttnArgs b;
        b.q = m->qd;
        b.ldq = d;
        b.k = m->ast_kvx[l];
        b.v = (const unsigned char*)m->ast_kvx[l] + (size_t)d * m->es;
        b.o = m->ctx;
        b.ldo = d;
        b.n = n;
        b.H = H;
        b.nkeys = m->Tp;
        b.d = d;
        b.utt = r.utt;
        b.keymask = m->keymask;
        b.scale = scale;
        ProfScope ps(m, "ast_src_attention", 4.0 * n * H * m->Tp * 64, 2.0 * n * m->Tp * d * m->es, s);
        CN_TRY(launch_ast_gather_attn(m->prec, 1, b, s));
    }
    return run_linear(m, "out_proj_resid", L.src_o, m->ctx, d, x, d, 1, n, CN_EPI_RESID, x, d, s);
}

// The newest position of the rows through the stack: st.x (the embedded tokens) -> final_norm of the stack's output in
// st.final_out.  Per layer: LN, fused QKV, cache attention over the earlier positions (it appends this position's K | V itself:
// it is the only reader of that row now), out-projection + residual, the source-attention sublayer of a layer that has one, the
// feed-forward sublayer.
int run_step_stack(cn_model* m, const StepStack& st, const StepRows& r, hipStream_t s) {
    const int d = m->cfg.d_model, H = m->cfg.n_head, n = r.n;
    const float scale = 1.0f / sqrtf((float)(d / H));
    float* x = st.x;
    bool have_ln = false;  // m->xn already holds LN(x) for the sublayer about to start
    for (size_t l = 0; l < st.layers.size(); ++l) {
        const Layer& L = st.layers[l];
        if (!have_ln) CN_TRY(run_ln(m, L.n[0], x, m->xn, n, s));
        CN_TRY(run_linear(m, st.tag_qkv, L.qkv, m->xn, d, m->qkv, 3 * d, 0, n, 0, nullptr, 0, s));
        GatherArgs g;
        g.q = m->qkv;
        g.ldq = 3 * d;
        g.k = m->ast_ck[l];
        g.v = m->ast_cv[l];
        g.o = m->ctx;
        g.ldo = d;
        g.n = n;
        g.H = H;
        g.d = d;
        g.table_stride = r.table_stride;
        g.scale = scale;
        {
            ProfScope ps(m, r.row_pos ? st.tag_attn_rows : st.tag_attn, 4.0 * n * H * (r.pos + 1) * 64, 2.0 * n * (r.pos + 1) * d * m->es, s);
            if (r.row_pos) {
                GatherRowsArgs a;
                static_cast<GatherArgs&>(a) = g;
                a.max_keys = r.pos + 1;
                a.rowid = r.anc;
                a.pos = r.row_pos;
                a.stay = r.row_stay;
                CN_TRY(launch_ast_gather_attn_rows(m->prec, a, s));
            } else {
                GatherAttnArgs a;
                static_cast<GatherArgs&>(a) = g;
                a.append_pos = r.pos;
                a.nkeys = r.pos + 1;
                a.slots = m->ast_slots;
                a.anc = r.anc;
                a.keyok = r.keyok;
                CN_TRY(launch_ast_gather_attn(m->prec, 0, a, s));
            }
        }
        CN_TRY(run_linear(m, st.tag_out, L.self_o, m->ctx, d, x, d, 1, n, CN_EPI_RESID, x, d, s));
        if (L.has_src) CN_TRY(run_src_attn_step(m, L, l, x, r, scale, s));
        const bool last = l + 1 == st.layers.size();
        CN_TRY(run_ffn_step(m, L, L.n[st.ffn_norm], x, n, last ? st.final_norm : st.layers[l + 1].n[0], last ? st.final_out : m->xn,
                            st.tag_ffn_split, s, &have_ln));
    }
    if (!have_ln) CN_TRY(run_ln(m, st.final_norm, x, st.final_out, n, s));
    return 0;
}
}  // namespace

// TransformerLM (src/models/lm.py:52-56) on the newest position of n hypotheses -> logits [n][V] fp32 in lm->ast_logits.  The
// reference runs lm_model(ys, tgt_mask) on the whole prefix under the decoder's mask (ys != padding_idx) & subsequent_mask
// (transformer.py:186-191); here the keys / values of earlier positions come from the LM's own cache through the SAME ancestor
// and key-mask tables as the decoder's.  The embedding, its pre-norm encoder layers as a step stack, then encoder.norm and
// out_generator.proj.
// With row_pos / row_stay (the CTC prefix beam search, whose hypotheses differ in length): row h sits at position row_pos[h] <= pos,
// anc_dev holds its cache ROW ids (one per prefix position, any row of the cache), every key is allowed (keyok_dev unused), and a
// row with row_stay[h] != 0 appends nothing - its logits are garbage the caller discards.
int lm_step_run(cn_model* lm, int n, int pos, const int32_t* tok_dev, const int32_t* anc_dev, const uint8_t* keyok_dev,
                int table_stride, hipStream_t s, const int32_t* row_pos, const int32_t* row_stay) {
    const int d = lm->cfg.d_model, V = lm->cfg.vocab_size;
    if (row_pos)
        CN_TRY(launch_ast_embed_rows(tok_dev, lm->tgt_lut, lm->pe, row_pos, lm->x, n, d, sqrtf((float)d), pos, s));
    else
        CN_TRY(launch_ast_embed(tok_dev, lm->tgt_lut, lm->pe + (size_t)pos * d, lm->x, n, d, sqrtf((float)d), s));
    const StepStack st{lm->enc, 1, lm->enc_norm, lm->enc_h, lm->x, "lm_qkv_proj", "lm_cache_attention", "lm_cache_attention_rows",
                       "lm_out_proj_resid", "lm_ffn_split"};
    CN_TRY(run_step_stack(lm, st, StepRows{n, pos, anc_dev, keyok_dev, table_stride, row_pos, row_stay}, s));
    return run_linear(lm, "lm_generator_proj", lm->att_gen, lm->enc_h, d, lm->ast_logits, V, 1, n, 0, nullptr, 0, s);
}
}  // namespace cn_host

// src/tasks/art_task.py:67-90 + transformer.py:186-209: the LM whose step ast_step fuses when lm_weight > 0 (NULL detaches).
extern "C" int cn_ast_attach_lm(cn_model* m, cn_model* lm) {
    if (!m || m->cfg.ast != 1) {
        cn_set_error("cn_ast_attach_lm: the first handle must be an autoregressive model (cfg.ast = 1)");
        return -1;
    }
    if (!lm) {
        m->ast_lm = nullptr;
        return 0;
    }
    CN_TRY(lm_check_pair(m, lm, "cn_ast_attach_lm"));
    m->ast_lm = lm;
    return 0;
}

extern "C" int cn_ast_begin(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                            int32_t want_ctc, int32_t max_len, int32_t max_slots, int32_t ctc_beam, void* stream) {
    CN_TRY(check_call(m, B, T, F));
    if (m->cfg.ast != 1 || !m->tgt_lut) {
        cn_set_error("cn_ast_begin: the model was not created with cfg.ast = 1");
        return -1;
    }
    if (max_len < 2 || max_slots < 1 || (size_t)max_slots > (size_t)m->maxB * (m->maxTp + 1) || ctc_beam < 0 || ctc_beam > 32) {
        cn_set_error("cn_ast_begin: bad max_len / max_slots / ctc_beam");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(ast_prepare_buffers(m, max_len, max_slots, ctc_beam));
    if (m->ast_lm) {  // the attached LM's step cache, sized like the decoder's
        CN_TRY(lm_check_step(m->ast_lm, max_len, max_slots, "cn_ast_begin"));
        CN_TRY(lm_prepare_buffers(m->ast_lm, max_len, max_slots));
    }
    m->ast_blank = opts->padding_idx;
    CN_TRY(stage_encode(m, feats_dev, B, T, F, opts, s));
    const int d = m->cfg.d_model, Mmem = B * m->Tp, V = m->cfg.vocab_size;
    for (size_t l = 0; l < m->mad.size(); ++l)  // cross-attention K|V of the memory, once per utterance batch
        CN_TRY(run_linear(m, "src_kv_proj", m->mad[l].src_kv, m->enc_h, d, m->ast_kvx[l], 2 * d, 0, Mmem, 0, nullptr, 0, s));
    if (want_ctc) {
        CN_TRY(run_linear(m, "generator_proj", m->ctc_gen, m->enc_h, d, m->logits, V, 1, Mmem, 0, nullptr, 0, s));
        CN_TRY(launch_logsoftmax_argmax(m->logits, Mmem, V, V, m->best, m->ctc_maxlp, 1, s));
        m->ctc_maxlp_valid = true;
        CN_TRY(launch_ast_ctc_prepare(m->logits, m->keymask, m->ast_r0, B, m->Tp, V, opts->padding_idx, s));
    }
    return 0;
}

namespace cn_host {
namespace {
// phrase biasing without CTC: where the rows' nodes come from (the caller's, or carried from the step before) in the fused top-K
struct AstBiasRows {
    const int32_t* node = nullptr;
    AbCarry carry;
};

// decoder layers on the newest position of n hypotheses -> top-K (token, temperature log-softmax value) per hypothesis
// dense_bw > 0: the rows are the dense slots b * dense_bw + j of the device beam (utt[row] = row / dense_bw)
int ast_step_run(cn_model* m, int n, int pos, const int32_t* tok_dev, const int32_t* utt_dev, const int32_t* anc_dev,
                 const uint8_t* keyok_dev, int table_stride, float temperature, int K, int32_t* topk_idx_dev,
                 float* topk_val_dev, int dense_bw, hipStream_t s, float lm_weight = 0.f, float* lm_val_dev = nullptr,
                 const float* ng_adds_dev = nullptr, int ng_eos = -1, const AstBiasRows* bias = nullptr) {
    const int d = m->cfg.d_model, V = m->cfg.vocab_size;
    CN_TRY(launch_ast_embed(tok_dev, m->tgt_lut, m->pe + (size_t)pos * d, m->xd, n, d, sqrtf((float)d), s));
    // DecoderLayer: self attention over the cached prefix, source attention over the memory, feed-forward
    const StepStack st{m->mad, 2, m->dec_norm, m->dec_h, m->xd, "qkv_proj", "ast_cache_attention", "ast_cache_attention",
                       "out_proj_resid", "ffn_split"};
    CN_TRY(run_step_stack(m, st, StepRows{n, pos, anc_dev, keyok_dev, table_stride, nullptr, nullptr, utt_dev, dense_bw}, s));
    CN_TRY(run_linear(m, "generator_proj", m->att_gen, m->dec_h, d, m->ast_logits, V, 1, n, 0, nullptr, 0, s));
    if (lm_weight > 0.f) {  // shallow fusion (transformer.py:186-209): the LM step on the same rows, tables and position
        cn_model* lm = m->ast_lm;
        CN_TRY(lm_step_run(lm, n, pos, tok_dev, anc_dev, keyok_dev, table_stride, s));
        ProfScope ps(m, "lm_fusion", 0, 2.0 * n * V * 4, s);
        if (!lm_val_dev)  // no CTC: top-K of att + lm_weight * lm over the vocabulary
            return launch_logsoftmax_fuse_topk(m->ast_logits, lm->ast_logits, n, V, V, temperature, lm_weight, K, topk_idx_dev,
                                               topk_val_dev, s);
        CN_TRY(launch_logsoftmax_topk(m->ast_logits, n, V, V, temperature, K, topk_idx_dev, topk_val_dev, s));
        return launch_logsoftmax_gather(lm->ast_logits, n, V, V, topk_idx_dev, K, lm_val_dev, s);
    }
    if (ng_adds_dev) {  // word n-gram fusion without CTC: top-K of att + scale * term(class of the token) over the vocabulary
        ProfScope ps(m, "ngram_fusion", 0, 1.0 * n * V * 4, s);
        return launch_logsoftmax_class_topk(m->ast_logits, n, V, V, temperature, m->ast_ng.piece_starts, ng_adds_dev, ng_eos,
                                            m->ast_ng_scale, K, topk_idx_dev, topk_val_dev, s);
    }
    if (bias) {  // phrase biasing without CTC: top-K of att + term(node of the row, token) over the vocabulary
        ProfScope ps(m, "bias_fusion", 0, 1.0 * n * V * 4, s);
        return launch_logsoftmax_bias_topk(m->ast_logits, n, V, V, temperature, m->ast_bias, bias->node, bias->carry, ng_eos, K,
                                           topk_idx_dev, topk_val_dev, s);
    }
    CN_TRY(launch_logsoftmax_topk(m->ast_logits, n, V, V, temperature, K, topk_idx_dev, topk_val_dev, s));
    return 0;
}
}  // namespace
}  // namespace cn_host

extern "C" int cn_ast_step(cn_model* m, int32_t n, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev,
                           const int32_t* anc_dev, const uint8_t* keyok_dev, int32_t table_stride, float temperature,
                           int32_t K, int32_t* topk_idx_dev, float* topk_val_dev, void* stream) {
    if (!m || !m->cfg.ast || m->ast_slots == 0) {
        cn_set_error("cn_ast_step: call cn_ast_begin first");
        return -1;
    }
    CN_TRY(step_check(m, "cn_ast_step", n, pos, table_stride, K < 1 ? -1 : K));  // (a K of 0 is not "no top-K" here)
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    return ast_step_run(m, n, pos, tok_dev, utt_dev, anc_dev, keyok_dev, table_stride, temperature, K, topk_idx_dev, topk_val_dev, 0,
                        (hipStream_t)stream);
}

extern "C" int cn_ast_step_lm(cn_model* m, int32_t n, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev,
                              const int32_t* anc_dev, const uint8_t* keyok_dev, int32_t table_stride, float temperature, int32_t K,
                              float lm_weight, int32_t use_ctc, int32_t* topk_idx_dev, float* topk_val_dev, float* lm_val_dev,
                              void* stream) {
    if (!m || m->cfg.ast != 1 || m->ast_slots == 0) {
        cn_set_error("cn_ast_step_lm: call cn_ast_begin first");
        return -1;
    }
    if (m->ast_ng_on) {
        cn_set_error("cn_ast_step_lm: an n-gram model is attached (cn_ast_attach_ngram); it and a TransformerLM cannot be fused together");
        return -1;
    }
    if (m->ast_bias_on) {
        cn_set_error("cn_ast_step_lm: a phrase list is attached (cn_ast_attach_bias); it and a TransformerLM cannot be fused together");
        return -1;
    }
    if (!(lm_weight > 0.f) || !m->ast_lm || m->ast_lm->ast_slots < m->ast_slots || m->ast_lm->ast_max_len < m->ast_max_len) {
        cn_set_error("cn_ast_step_lm: needs lm_weight > 0 and an LM attached (cn_ast_attach_lm) before cn_ast_begin");
        return -1;
    }
    CN_TRY(step_check(m, "cn_ast_step_lm", n, pos, table_stride, K < 1 ? -1 : K));
    if (use_ctc && !lm_val_dev) {
        cn_set_error("cn_ast_step_lm: use_ctc without lm_val_dev");
        return -1;
    }
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    return ast_step_run(m, n, pos, tok_dev, utt_dev, anc_dev, keyok_dev, table_stride, temperature, K, topk_idx_dev, topk_val_dev, 0,
                        (hipStream_t)stream, lm_weight, use_ctc ? lm_val_dev : nullptr);
}

// include/cassnat_hip_ast_ngram.h: the word n-gram model whose class terms the step fuses (NULL detaches)
extern "C" int cn_ast_attach_ngram(cn_model* m, const cn_ngram_desc* desc, float lm_scale) {
    if (!m || m->cfg.ast != 1) {
        cn_set_error("cn_ast_attach_ngram: the handle must be an autoregressive model (cfg.ast = 1)");
        return -1;
    }
    if (!desc) {
        m->ast_ng_on = false;
        m->ast_ng = cn_ngram_desc{};
        m->ast_ng_scale = 0.f;
        return 0;
    }
    const std::string bad = ng_check_desc(*desc);
    if (!bad.empty()) {
        cn_set_error("cn_ast_attach_ngram: " + bad);
        return -1;
    }
    if (desc->vocab != m->cfg.vocab_size) {
        cn_set_error("cn_ast_attach_ngram: the model's pieces must be the decoder's vocabulary (desc->vocab " + std::to_string(desc->vocab) +
                     ", vocab_size " + std::to_string(m->cfg.vocab_size) + ")");
        return -1;
    }
    if (!(lm_scale == lm_scale)) {
        cn_set_error("cn_ast_attach_ngram: lm_scale must be a number");
        return -1;
    }
    if (m->ast_bias_on) {
        cn_set_error("cn_ast_attach_ngram: a phrase list is attached (cn_ast_attach_bias); it and an n-gram model cannot be fused together");
        return -1;
    }
    m->ast_ng = *desc;
    m->ast_ng_scale = lm_scale;
    m->ast_ng_on = true;
    return 0;
}

extern "C" int cn_ast_step_ngram(cn_model* m, int32_t n, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev,
                                 const int32_t* anc_dev, const uint8_t* keyok_dev, int32_t table_stride, float temperature, int32_t K,
                                 int32_t use_ctc, int32_t eos, const float* adds_dev, int32_t* topk_idx_dev, float* topk_val_dev,
                                 float* term_dev, void* stream) {
    if (!m || m->cfg.ast != 1 || m->ast_slots == 0) {
        cn_set_error("cn_ast_step_ngram: call cn_ast_begin first");
        return -1;
    }
    if (!m->ast_ng_on) {
        cn_set_error("cn_ast_step_ngram: needs an n-gram model attached with cn_ast_attach_ngram");
        return -1;
    }
    if (m->ast_lm) {
        cn_set_error("cn_ast_step_ngram: an n-gram model and a TransformerLM are attached together; detach one");
        return -1;
    }
    CN_TRY(step_check(m, "cn_ast_step_ngram", n, pos, table_stride, K < 1 ? -1 : K));
    if (!adds_dev || (use_ctc && !term_dev)) {
        cn_set_error("cn_ast_step_ngram: no adds_dev, or use_ctc without term_dev");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(ast_step_run(m, n, pos, tok_dev, utt_dev, anc_dev, keyok_dev, table_stride, temperature, K, topk_idx_dev, topk_val_dev, 0, s,
                        0.f, nullptr, use_ctc ? nullptr : adds_dev, eos));
    if (use_ctc) return launch_ast_ngram_terms(m->ast_ng.piece_starts, adds_dev, eos, topk_idx_dev, n, K, term_dev, s);
    return 0;
}

// include/cassnat_hip_ast_bias.h: the phrase list whose terms the step fuses (NULL detaches)
extern "C" int cn_ast_attach_bias(cn_model* m, const cn_bias_desc* desc) {
    if (!m || m->cfg.ast != 1) {
        cn_set_error("cn_ast_attach_bias: the handle must be an autoregressive model (cfg.ast = 1)");
        return -1;
    }
    if (!desc) {
        m->ast_bias_on = false;
        m->ast_bias = cn_bias_desc{};
        return 0;
    }
    const std::string bad = cb_check_desc(*desc);
    if (!bad.empty()) {
        cn_set_error("cn_ast_attach_bias: " + bad);
        return -1;
    }
    if (m->ast_ng_on) {
        cn_set_error("cn_ast_attach_bias: an n-gram model is attached (cn_ast_attach_ngram); it and a phrase list cannot be fused together");
        return -1;
    }
    m->ast_bias = *desc;
    m->ast_bias_on = true;
    return 0;
}

extern "C" int cn_ast_step_bias(cn_model* m, int32_t n, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev,
                                const int32_t* anc_dev, const uint8_t* keyok_dev, int32_t table_stride, float temperature, int32_t K,
                                int32_t use_ctc, int32_t eos, const int32_t* node_dev, int32_t* topk_idx_dev, float* topk_val_dev,
                                float* term_dev, void* stream) {
    if (!m || m->cfg.ast != 1 || m->ast_slots == 0) {
        cn_set_error("cn_ast_step_bias: call cn_ast_begin first");
        return -1;
    }
    if (!m->ast_bias_on) {
        cn_set_error("cn_ast_step_bias: needs a phrase list attached with cn_ast_attach_bias");
        return -1;
    }
    if (m->ast_lm) {
        cn_set_error("cn_ast_step_bias: a phrase list and a TransformerLM are attached together; detach one");
        return -1;
    }
    CN_TRY(step_check(m, "cn_ast_step_bias", n, pos, table_stride, K < 1 ? -1 : K));
    if (!node_dev || (use_ctc && !term_dev)) {
        cn_set_error("cn_ast_step_bias: no node_dev, or use_ctc without term_dev");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    AstBiasRows rows;
    rows.node = node_dev;
    CN_TRY(ast_step_run(m, n, pos, tok_dev, utt_dev, anc_dev, keyok_dev, table_stride, temperature, K, topk_idx_dev, topk_val_dev, 0, s,
                        0.f, nullptr, nullptr, eos, use_ctc ? nullptr : &rows));
    if (use_ctc) return launch_ast_bias_terms(m->ast_bias, node_dev, AbCarry{}, eos, topk_idx_dev, n, K, term_dev, s);
    return 0;
}

// kernel-test entry of the LM step: log_softmax of the LM's logits at position pos of n rows -> logp_dev [n][V]
extern "C" int cn_lm_step_begin(cn_model* lm, int32_t max_len, int32_t max_slots) {
    CN_TRY(lm_check_step(lm, max_len, max_slots, "cn_lm_step_begin"));
    if (max_len < 1 || max_slots < 1) {
        cn_set_error("cn_lm_step_begin: bad max_len / max_slots");
        return -1;
    }
    CN_HIP_CHECK(hipSetDevice(lm->cfg.device));
    return lm_prepare_buffers(lm, max_len, max_slots);
}

extern "C" int cn_lm_step(cn_model* lm, int32_t n, int32_t pos, const int32_t* tok_dev, const int32_t* anc_dev,
                          const uint8_t* keyok_dev, int32_t table_stride, float* logp_dev, void* stream) {
    if (!lm || lm->cfg.ast != 2 || lm->ast_slots == 0) {
        cn_set_error("cn_lm_step: call cn_lm_step_begin first");
        return -1;
    }
    CN_TRY(step_check(lm, "cn_lm_step", n, pos, table_stride, 0));
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(lm->cfg.device));
    const int V = lm->cfg.vocab_size;
    CN_TRY(lm_step_run(lm, n, pos, tok_dev, anc_dev, keyok_dev, table_stride, s));
    CN_TRY(launch_logsoftmax_argmax(lm->ast_logits, n, V, V, lm->best, lm->ctc_maxlp, 1, s));
    CN_HIP_CHECK(hipMemcpyAsync(logp_dev, lm->ast_logits, (size_t)n * V * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// kernel-test entry of the LM step with a position per row (cn_ctc_beam_lm's): row h holds token tok_dev[h] at position
// pos_dev[h] <= max_pos; rowid_dev [n][table_stride] names the cache row of every prefix position (any row below the
// max_len * max_slots of cn_lm_step_begin; the caller keeps them in range - they are not read back here); rows with stay_dev[h]
// != 0 append nothing and their output is unspecified.  logp_dev [n][V]: log_softmax of the logits, as cn_lm_step's.
extern "C" int cn_lm_step_rows(cn_model* lm, int32_t n, int32_t max_pos, const int32_t* tok_dev, const int32_t* pos_dev,
                               const int32_t* stay_dev, const int32_t* rowid_dev, int32_t table_stride, float* logp_dev, void* stream) {
    if (!lm || lm->cfg.ast != 2 || lm->ast_slots == 0) {
        cn_set_error("cn_lm_step_rows: call cn_lm_step_begin first");
        return -1;
    }
    if (!tok_dev || !pos_dev || !stay_dev || !rowid_dev || !logp_dev) {
        cn_set_error("cn_lm_step_rows: null array");
        return -1;
    }
    CN_TRY(step_check(lm, "cn_lm_step_rows", n, max_pos, table_stride, 0));
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(lm->cfg.device));
    const int V = lm->cfg.vocab_size;
    CN_TRY(lm_step_run(lm, n, max_pos, tok_dev, rowid_dev, nullptr, table_stride, s, pos_dev, stay_dev));
    CN_TRY(launch_logsoftmax_argmax(lm->ast_logits, n, V, V, lm->best, lm->ctc_maxlp, 1, s));
    CN_HIP_CHECK(hipMemcpyAsync(logp_dev, lm->ast_logits, (size_t)n * V * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

extern "C" int cn_ast_ctc_score(cn_model* m, int32_t n, int32_t out_len, const int32_t* utt_dev, const int32_t* last_tok_dev,
                                const int32_t* cand_dev, int32_t K, const int32_t* prev_ref_dev, int32_t parity, int32_t eos,
                                float* score_dev, void* stream) {
    if (!m || !m->cfg.ast || !m->ast_r0 || K < 1 || K > m->ast_ctc_beam || n < 1 || n > m->ast_slots) {
        cn_set_error("cn_ast_ctc_score: call cn_ast_begin with want_ctc and a ctc_beam >= K first");
        return -1;
    }
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CtcPrefixArgs a;
    a.logp = m->logits;
    a.r0 = m->ast_r0;
    a.r_prev = m->ast_r[(parity & 1) ^ 1];
    a.r_new = m->ast_r[parity & 1];
    a.utt = utt_dev;
    a.last_tok = last_tok_dev;
    a.cand = cand_dev;
    a.prev_ref = prev_ref_dev;
    a.score = score_dev;
    a.n = n;
    a.K = K;
    a.Tp = m->Tp;
    a.V = m->cfg.vocab_size;
    a.blank = m->ast_blank;
    a.eos = eos;
    a.out_len = out_len;
    return launch_ast_ctc_prefix(a, (hipStream_t)stream);
}

// Whole joint CTC/attention beam search on the device (transformer.py:122-241): encoder, then max_step iterations of
// [decoder step on every slot -> CTC prefix scores -> beam update kernel]; the host only polls the live-hypothesis
// counter every 8 steps to stop early.  Outputs (device pointers): hyp_out [B][beam_width][max_len] (sos first, padded
// with padding_idx), hyp_len [B][beam_width], score [B][beam_width] as double; beams best first.
extern "C" int cn_decode_ast(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                             const cn_ast_opts* ao, int32_t* hyp_out_dev, int32_t max_len, int32_t* hyp_len_dev,
                             double* score_dev, void* stream) {
    if (!m || !opts || !ao || !hyp_out_dev || !hyp_len_dev || !score_dev) {
        cn_set_error("cn_decode_ast: null argument");
        return -1;
    }
    const int bw = ao->beam_width, want_ctc = ao->ctc_weight > 0.f ? 1 : 0;
    const int K = want_ctc ? ao->ctc_beam : bw;
    if (bw < 1 || bw > 32 || K < bw || K > 32 || ao->max_step < 1 || max_len < ao->max_step + 1) {
        cn_set_error("cn_decode_ast: need 1 <= beam_width <= ctc_beam <= 32 and max_len > max_step");
        return -1;
    }
    if (K > m->cfg.vocab_size) {
        cn_set_error("cn_decode_ast: the candidate count (ctc_beam, or beam_width without CTC) exceeds the vocabulary");
        return -1;
    }
    // step pos scores prefixes of pos tokens: the CTC prefix scorer is defined up to out_len == T' (the reference raises
    // IndexError beyond it), so the last step, max_step - 1, must not pass the subsampled frame count
    const int Tp = ((T - 1) / 2 + 1 - 1) / 2 + 1;
    if (want_ctc && ao->max_step > Tp + 1) {
        cn_set_error("cn_decode_ast: with CTC, max_step may not exceed the subsampled frame count + 1 (max_decode_ratio too large: "
                     "the CTC prefix score of a hypothesis longer than the frames is undefined)");
        return -1;
    }
    const bool use_lm = ao->lm_weight > 0.f;
    if (use_lm && !m->ast_lm) {
        cn_set_error("cn_decode_ast: lm_weight > 0 needs an LM attached with cn_ast_attach_lm");
        return -1;
    }
    const bool use_ng = m->ast_ng_on;
    if (use_ng && use_lm) {
        cn_set_error("cn_decode_ast: an n-gram model is attached and lm_weight > 0 asks for the TransformerLM; the two cannot be fused together");
        return -1;
    }
    const bool use_bias = m->ast_bias_on;
    if (use_bias && (use_lm || m->ast_lm)) {
        cn_set_error("cn_decode_ast: a phrase list is attached (cn_ast_attach_bias) beside a TransformerLM; the two cannot be fused together");
        return -1;
    }
    if (use_bias && use_ng) {
        cn_set_error("cn_decode_ast: a phrase list and an n-gram model are attached together; detach one");
        return -1;
    }
    const int S = B * bw, L = max_len;
    CN_TRY(cn_ast_begin(m, feats_dev, B, T, F, opts, want_ctc, L, S, want_ctc ? K : 0, stream));
    hipStream_t s = (hipStream_t)stream;
    if (m->beam_S < S || m->beam_L < L || m->beam_K < K) {
        AstBeamState& st = m->beam;
        for (int i = 0; i < 2; ++i) {
            CN_TRY(ast_alloc(m, (void**)&st.tok[i], (size_t)S * L * 4));
            CN_TRY(ast_alloc(m, (void**)&st.anc[i], (size_t)S * L * 4));
            CN_TRY(ast_alloc(m, (void**)&st.keyok[i], (size_t)S * L));
            CN_TRY(ast_alloc(m, (void**)&st.len[i], (size_t)S * 4));
            CN_TRY(ast_alloc(m, (void**)&st.score[i], (size_t)S * 8));
            CN_TRY(ast_alloc(m, (void**)&st.valid[i], (size_t)S * 4));
            CN_TRY(ast_alloc(m, (void**)&st.ctc_ref[i], (size_t)S * 4));
            CN_TRY(ast_alloc(m, (void**)&st.ctc_prev[i], (size_t)S * 4));
        }
        CN_TRY(ast_alloc(m, (void**)&st.cur_tok, (size_t)S * 4));
        CN_TRY(ast_alloc(m, (void**)&st.utt, (size_t)S * 4));
        CN_TRY(ast_alloc(m, (void**)&st.live, 64));
        CN_TRY(ast_alloc(m, (void**)&m->beam_idx, (size_t)S * K * 4));
        CN_TRY(ast_alloc(m, (void**)&m->beam_val, (size_t)S * K * 4));
        CN_TRY(ast_alloc(m, (void**)&m->beam_ctc, (size_t)S * K * 4));
        CN_TRY(ast_alloc(m, (void**)&m->beam_lm, (size_t)S * K * 4));
        CN_TRY(ast_alloc(m, (void**)&m->beam_adds, (size_t)S * 2 * 4));
        for (int i = 0; i < 2; ++i) CN_TRY(ast_alloc(m, (void**)&m->beam_node[i], (size_t)S * 4));
        m->beam_S = S;
        m->beam_L = L;
        m->beam_K = K;
    }
    const AstBeamState& st = m->beam;
    int cur = 0;
    CN_TRY(launch_ast_beam_init(st, cur, B, bw, L, opts->sos, opts->padding_idx, s));
    for (int pos = 0; pos < ao->max_step; ++pos) {
        // word n-gram fusion: every slot's (a_word, a_eos) from its own tokens behind sos.  Without CTC they enter the top-K over the
        // vocabulary; with CTC the same launch runs behind the attention top-K and writes the terms at its candidates
        if (use_ng && !want_ctc)
            CN_TRY(launch_ast_ngram_adds(m->ast_ng, st.tok[cur], L, 1, st.len[cur], -1, S, ao->eos, m->beam_adds, nullptr, 0, nullptr, s));
        // phrase biasing: a slot's node is one cb_step from the node of the slot that computed the position before (the ancestor table
        // names it, as it does for the KV cache); the launch that needs it - the fused top-K without CTC, the terms with CTC - computes
        // it and keeps it for the next step
        AstBiasRows brows;
        if (use_bias) {
            AbCarry& c = brows.carry;
            c.prev = pos > 0 ? m->beam_node[(pos & 1) ^ 1] : nullptr;
            c.anc = st.anc[cur];
            c.tok = st.cur_tok;
            c.out = m->beam_node[pos & 1];
            c.ld = L, c.col = pos - 1, c.slots = S;
        }
        CN_TRY(ast_step_run(m, S, pos, st.cur_tok, st.utt, st.anc[cur], st.keyok[cur], L, ao->temperature, K, m->beam_idx,
                            m->beam_val, bw, s, use_lm ? ao->lm_weight : 0.f, use_lm && want_ctc ? m->beam_lm : nullptr,
                            use_ng && !want_ctc ? m->beam_adds : nullptr, ao->eos, use_bias && !want_ctc ? &brows : nullptr));
        if (use_ng && want_ctc)
            CN_TRY(launch_ast_ngram_adds(m->ast_ng, st.tok[cur], L, 1, st.len[cur], -1, S, ao->eos, m->beam_adds, m->beam_idx, K,
                                         m->beam_lm, s));
        if (use_bias && want_ctc)
            CN_TRY(launch_ast_bias_terms(m->ast_bias, nullptr, brows.carry, ao->eos, m->beam_idx, S, K, m->beam_lm, s));
        if (want_ctc)
            CN_TRY(cn_ast_ctc_score(m, S, pos, st.utt, st.cur_tok, m->beam_idx, K, st.ctc_ref[cur], pos & 1, ao->eos, m->beam_ctc,
                                    stream));
        AstBeamStep q;
        q.idx = m->beam_idx;
        q.att = m->beam_val;
        q.ctc = m->beam_ctc;
        q.cur = cur;
        q.pos = pos;
        q.bw = bw;
        q.K = K;
        q.L = L;
        q.eos = ao->eos;
        q.sos = opts->sos;
        q.pad = opts->padding_idx;
        q.use_ctc = want_ctc;
        q.use_lp = ao->use_length_penalty;
        q.use_lm = use_lm || use_ng || use_bias;
        q.lm = m->beam_lm;
        q.lw = use_bias ? 1.0f : (use_ng ? m->ast_ng_scale : ao->lm_weight);
        q.w = ao->ctc_weight;
        q.u = ao->one_minus_ctc_weight;
        q.lp = ao->length_penalty;
        CN_TRY(launch_ast_beam_update(st, q, B, s));
        cur ^= 1;
        if ((pos & 7) == 7 && pos + 1 < ao->max_step) {  // every 8 steps: anything still alive?
            CN_HIP_CHECK(hipMemcpyAsync(m->ymax_pinned + 8, st.live, sizeof(int), hipMemcpyDeviceToHost, s));
            CN_HIP_CHECK(hipStreamSynchronize(s));
            if (m->ymax_pinned[8] == 0) break;
        }
    }
    CN_HIP_CHECK(hipMemcpyAsync(hyp_out_dev, st.tok[cur], (size_t)S * L * 4, hipMemcpyDeviceToDevice, s));
    CN_HIP_CHECK(hipMemcpyAsync(hyp_len_dev, st.len[cur], (size_t)S * 4, hipMemcpyDeviceToDevice, s));
    CN_HIP_CHECK(hipMemcpyAsync(score_dev, st.score[cur], (size_t)S * 8, hipMemcpyDeviceToDevice, s));
    return 0;
}

