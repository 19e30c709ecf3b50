// The sublayer building blocks of every decode pipeline (run_linear .. run_generator): each brackets the launches of one
// kernel tag for the profiler and fills the launcher's argument struct from the handle's weight views and workspace.
#include <algorithm>
#include <cmath>

#include "model.h"

namespace cn_host {

int run_linear(cn_model* m, const char* tag, const Linear& l, const void* A, int lda, void* C, int ldc, int c_f32, int M,
               int epi, const float* resid, int ldr, hipStream_t s) {
    ProfScope ps(m, tag, 2.0 * M * l.N * l.K,
                 (double)M * l.K * m->es + (double)l.N * l.K * m->es + (double)M * l.N * (c_f32 ? 4 : m->es), s);
    static const bool no_proj_x3 = cn_exp_env("CASSNAT_NO_PROJ_X3") != nullptr;
    if (l.px3 && m->prec == CN_PREC_X3 && !no_proj_x3 && (epi == 0 || epi == CN_EPI_RESID) && (epi == 0 || c_f32) && lda % 32 == 0 &&
        (c_f32 || ldc % 32 == 0) && (long long)M * std::max(ldc, ldr) * 4 < (1ll << 31)) {
        ProjX3Args a;
        a.A = A;
        a.lda = lda;
        a.wp = l.px3;
        a.bias = l.b;
        a.C = C;
        a.ldc = ldc;
        a.c_f32 = c_f32;
        a.resid = epi == CN_EPI_RESID ? resid : nullptr;
        a.ldr = ldr;
        a.M = M;
        a.N = l.N;
        return launch_proj_x3(a, s);
    }
    GemmArgs g;
    g.A = A;
    g.lda = lda;
    g.W = l.W;
    g.bias = l.b;
    g.C = C;
    g.ldc = ldc;
    g.c_f32 = c_f32;
    g.M = M;
    g.N = l.N;
    g.K = l.K;
    g.epi = epi;
    g.resid = resid;
    g.ldr = ldr;
    return launch_gemm(m->prec, g, s);
}

int run_ln(cn_model* m, const Norm& n, const float* x, void* y, int M, hipStream_t s) {
    ProfScope ps(m, "layernorm", 0, (double)M * m->cfg.d_model * (4 + m->es), s);
    return launch_layernorm(m->prec, x, n.a, n.b, y, 0, M, m->cfg.d_model, 1e-6f, s);
}

// x += FFN(LN(x)); when `next` is given, next_out <- LN_next(x) in model precision (fused into the FFN kernel on
// the bf16/d256 path, a separate LayerNorm launch otherwise)
int run_ffn(cn_model* m, const Layer& L, const Norm& n, float* x, int M, const Norm* next, void* next_out,
            hipStream_t s) {
    const int d = m->cfg.d_model;
    if (L.wx3) {  // split-bf16 engine: LN + w_1 + ReLU / Swish + w_2 + residual (+ next LN) in one launch, 3 MFMAs per product
        ProfScope ps(m, "ffn_fused_x3", 4.0 * M * (double)L.w1.N * d,
                     (double)M * d * 8 + 2.0 * L.w1.N * d * 4 + (next ? (double)M * d * 4 : 0.0), s);
        FfnX3Args a;
        a.x = x;
        a.ln_a = n.a;
        a.ln_b = n.b;
        a.wst = L.wx3;
        a.mix = !L.ff_swish && ffn_mix_applies();  // (as Packer::ffn packed the stream: weights.hip)
        a.act = L.ff_swish ? FF_ACT_SWISH : FF_ACT_RELU;
        a.b1 = L.w1.b;
        a.b2 = L.w2.b;
        if (next) {
            a.nln_a = next->a;
            a.nln_b = next->b;
            a.xn_out = next_out;
        }
        a.M = M;
        a.d = d;
        a.dff = L.w1.N;
        return launch_ffn_x3(a, s);
    }
    if (L.w1p) {
        ProfScope ps(m, "ffn_fused", 4.0 * M * (double)L.w1.N * d,
                     (double)M * d * 8 + 2.0 * L.w1.N * d * 2 + (next ? (double)M * d * 2 : 0.0), s);
        FfnFusedArgs a;
        a.x = x;
        a.ln_a = n.a;
        a.ln_b = n.b;
        a.w1p = L.w1p;
        a.b1 = L.w1.b;
        a.w2p = L.w2p;
        a.b2 = L.w2.b;
        if (next) {
            a.nln_a = next->a;
            a.nln_b = next->b;
            a.xn_out = next_out;
        }
        a.M = M;
        a.d = d;
        a.dff = L.w1.N;
        a.act = L.ff_swish ? FF_ACT_SWISH : FF_ACT_RELU;
        return launch_ffn_fused(a, s);
    }
    CN_TRY(run_ln(m, n, x, m->xn, M, s));
    if (L.ff_swish)
        CN_TRY(run_linear(m, "ffn_w1_swish", L.w1, m->xn, d, m->hbuf, L.w1.N, 0, M, CN_EPI_SWISH, nullptr, 0, s));
    else
        CN_TRY(run_linear(m, "ffn_w1_relu", L.w1, m->xn, d, m->hbuf, L.w1.N, 0, M, CN_EPI_RELU, nullptr, 0, s));
    CN_TRY(run_linear(m, "ffn_w2_resid", L.w2, m->hbuf, L.w1.N, x, d, 1, M, CN_EPI_RESID, x, d, s));
    if (next) CN_TRY(run_ln(m, *next, x, next_out, M, s));
    return 0;
}

// Split-bf16 engine, the row-chain form of a self-attention layer's tail (fused_x3.hip, PRO / TAIL): in ONE launch behind the
// attention kernel  x += Wo . ctx + bo;  x += FFN(LN1 x);  then either LN_next(x) -> next_out (split-bf16 rows) or, with `tail`, the
// next attention's projection of it -> tail_out (the activations between the three products never leave LDS / registers).
bool x3_chain_applies(const cn_model* m, const Layer& L, const Linear* tail) {
    return m->prec == CN_PREC_X3 && L.wx3 && !L.ff_swish && L.self_o.px3 && L.self_o.N == 256 && L.self_o.K == 256 &&
           (!tail || (tail->px3 && tail->K == 256 && tail->N % 128 == 0 && tail->N <= 1024));
}
int run_x3_chain(cn_model* m, const Layer& L, const Norm& n1, float* x, int M, const Norm& next, void* next_out, const Linear* tail,
                 void* tail_out, int ld_tail, const char* tag, hipStream_t s) {
    const int d = m->cfg.d_model, tn = tail ? tail->N : 0;
    const double macs = (double)d * d + 2.0 * d * L.w1.N + (double)d * tn;
    ProfScope ps(m, tag, 2.0 * M * macs, (double)M * d * (4 + 8) + (double)M * (tail ? tn : d) * 4 + 4.0 * macs, s);
    FfnX3Args a;
    a.x = x;
    a.ln_a = n1.a;
    a.ln_b = n1.b;
    a.wst = L.wx3;
    a.mix = ffn_mix_applies();
    a.b1 = L.w1.b;
    a.b2 = L.w2.b;
    a.nln_a = next.a;
    a.nln_b = next.b;
    a.xn_out = next_out;
    a.M = M;
    a.d = d;
    a.dff = L.w1.N;
    a.ctx = m->ctx;
    a.ldctx = d;
    a.wo_p = L.self_o.px3;
    a.bo = L.self_o.b;
    if (tail) {
        a.tail_p = tail->px3;
        a.tail_b = tail->b;
        a.tail_out = tail_out;
        a.tail_n = tn;
        a.ld_tail = ld_tail;
    }
    return launch_ffn_x3(a, s);
}

// ctx <- Attn(q, k, v) on the fused [M][3d] projection buffer m->qkv
// row_off: packed rows (AttnArgs.row_off; queries AND keys are the entry's own rows) - the decoder side of a packed pass
// proj: the kernel projects Q | K | V itself (AttnArgs.proj_y) from LNn(x) in m->xn (the blocked ln_out of a run_chain launch
// with `ln_only`) and the tail units / biases of that launch's stream - m->qkv is neither written nor read
int run_self_attn_core(cn_model* m, int B, int Lseq, const unsigned char* keymask, const int* klen, int causal,
                       hipStream_t s, bool blocked, const int* row_off, const ChainRef* proj) {
    const int d = m->cfg.d_model, M = B * Lseq;
    AttnArgs a;
    const size_t es = m->es;
    a.Q = m->qkv;
    a.K = (const unsigned char*)m->qkv + (size_t)d * es;
    a.V = (const unsigned char*)m->qkv + (size_t)2 * d * es;
    if (blocked) {  // m->qkv as the row-chain kernel's tail wrote it: a blocked [M][3d] matrix
        a.K = a.V = m->qkv;
        a.q_blocked = a.kv_blocked = 1;
        a.q_col = 0;
        a.k_col = d;
        a.v_col = 2 * d;
        a.q_n = a.kv_n = 3 * d;
        a.o_blocked = 1;  // (blocked in = the row-chain path: its next launch reads ctx as B operands)
    }
    if (proj) {
        a.proj_y = m->xn;
        a.proj_w = (const unsigned char*)proj->w +
                   chain_stream_units(proj->has_wo, proj->dff, 0, proj->f8q != nullptr) * (size_t)CHAIN_UNIT_BYTES;
        a.proj_b = proj->tab + CHAIN_TAB_BT;
        a.o_blocked = 1;
    }
    m->ctx_blocked = a.o_blocked != 0;
    a.O = m->ctx;
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.ldo = d;
    a.B = B;
    a.H = m->cfg.n_head;
    a.Lq = a.Lk = Lseq;
    a.keymask = keymask;
    a.klen = klen;
    a.row_off = row_off;
    a.kv_packed = row_off ? 1 : 0;
    if (m->ragged && keymask == m->keymask) {  // encoder self-attention of a merged pass
        a.kcap = &m->utt_meta[0].tp;
        a.kcap_stride = (int)(sizeof(UttMeta) / sizeof(int));
    }
    a.causal = causal;
    a.scale = 1.0f / sqrtf((float)(d / m->cfg.n_head));
    // (projecting form: + the Q|K|V product; LNn(x) in and ctx out, and every (entry, head) workgroup its 6 tail units)
    ProfScope ps(m, "self_attention", 4.0 * B * a.H * (double)Lseq * Lseq * 64 + (proj ? 2.0 * M * d * 3.0 * d : 0.0),
                 proj ? (double)M * 2 * d * m->es + (double)B * 3 * d * d * m->es : (double)M * 4 * d * m->es, s);
    return launch_attention(m->prec, a, s);
}

// x += O(Attn(LN(x) Wq, LN(x) Wk, LN(x) Wv))
// `pre` == nullptr: m->xn already holds LN(x) (written by the preceding FFN)
int run_self_attn(cn_model* m, const Layer& L, const Norm* pre, float* x, int B, int Lseq, const unsigned char* keymask,
                  const int* klen, int causal, hipStream_t s) {
    const int d = m->cfg.d_model, M = B * Lseq;
    if (pre) CN_TRY(run_ln(m, *pre, x, m->xn, M, s));
    CN_TRY(run_linear(m, "qkv_proj", L.qkv, m->xn, d, m->qkv, 3 * d, 0, M, 0, nullptr, 0, s));
    CN_TRY(run_self_attn_core(m, B, Lseq, keymask, klen, causal, s));
    CN_TRY(run_linear(m, "out_proj_resid", L.self_o, m->ctx, d, x, d, 1, M, CN_EPI_RESID, x, d, s));
    return 0;
}

// row-chain launch: [x += Wo ctx + bo]; [x += FFN(LN1 x)]; [out <- tail projection of LNn(x) (or LNn(x) itself)].
// `with_next` false drops the norm/projection part of a stream that has one (use_unimask cuts the carry SAD -> MAD).
// x_mode: CHX_* bits (model.h)
// tag: the profile row of the launch ("row_chain": encoder-side, full-width launches; "row_chain_dec": the decoder side's - a
// tenth of the rows, a quarter of the CUs: bench.py prices the two apart)
// ln_only: the stream's tail projection is left to its reader (run_self_attn_core with `proj`) - the launch ends with LNn(x),
// written to `out` ([ceil(M / 32) * 32][d]) as the kernel's own B operands (ChainArgs.ln_blocked)
int run_chain(cn_model* m, const ChainRef& r, float* x, int M, void* out, int ldo, bool with_next, int x_mode,
              hipStream_t s, void* ln_out, int ld_ln, bool out_blocked, const char* tag, const int* m_dev, bool ln_only) {
    const int d = m->cfg.d_model;
    const int tail_n = with_next && !ln_only ? r.tail_n : 0;
    const double macs = (r.has_wo ? (double)d * d : 0.0) + 2.0 * d * r.dff + (double)d * tail_n;
    ProfScope ps(m, tag, 2.0 * M * macs, (double)M * d * (8 + 2) + (double)M * ldo * 2 + 2.0 * macs, s);
    ChainArgs a;
    a.x = x;
    a.ctx = r.has_wo ? m->ctx : nullptr;
    a.ldctx = d;
    a.ctx_blocked = m->ctx_blocked ? 1 : 0;  // (as the attention launch before this one wrote it)
    a.wstream = r.w;
    a.tab = r.tab;
    a.out = out;
    a.ldo = ldo;
    a.ln_out = ln_out;
    a.ld_ln = ld_ln;
    a.M = M;
    a.m_dev = m_dev;  // (packed decoder rows: M is the capacity, the device word the rows that exist)
    a.d = d;
    a.dff = r.dff;
    a.tail_n = tail_n;
    a.has_next = with_next && r.has_next;
    a.x_in_blocked = (x_mode & CHX_IN_BLK) != 0;
    a.x_out_blocked = (x_mode & CHX_OUT_BLK) != 0;
    a.store_x = (x_mode & CHX_NO_STORE) == 0;
    a.swish = r.swish ? 1 : 0;
    a.out_blocked = out_blocked ? 1 : 0;
    a.ln_blocked = ln_only ? 1 : 0;
    a.f8 = r.f8q ? 1 : 0;
    a.f8_q = r.f8q;
    return launch_chain(a, s);
}

// ---- encoder layer with e4m3fn products (BASELINE config 5; the layer of encoder.py / transformer_blocks.py) -------------
// Operands carry per-tensor power-of-two scales: the weights' is chosen at pack time (largest that keeps max|w| in range,
// stored beside them), the activations' are fixed - LayerNorm outputs and attention contexts x16 (saturating at 28), the
// ReLU hidden activations x8 (saturating at 56).  Accumulation, bias, residual and LayerNorm stay fp32; attention runs
// on the bf16 Q|K|V the first product writes.  LayerNorm and the first FFN product write their fp8 outputs directly; only
// the attention context needs a quantisation pass.
constexpr float FP8_S_LN = 16.f, FP8_S_CTX = 16.f, FP8_S_HID = 8.f;  // (FP8_S_IMG, the conv1 image's: model.h)
static int run_linear_fp8(cn_model* m, const char* tag, const Linear& l, const void* a8, float a_scale, void* C, int ldc, int c_f32,
                          int c_fp8, float c_scale, int M, int epi, const float* resid, int ldr, hipStream_t s) {
    ProfScope ps(m, tag, 2.0 * M * l.N * l.K, (double)M * l.K + (double)l.N * l.K + (double)M * l.N * (c_f32 ? 4 : (c_fp8 ? 1 : 2)), s);
    GemmArgs g;
    g.A = a8;
    g.lda = l.K;
    g.W = l.W8;
    g.bias = l.b;
    g.C = C;
    g.ldc = ldc;
    g.c_f32 = c_f32;
    g.c_fp8 = c_fp8;
    g.c_scale = c_scale;
    g.M = M;
    g.N = l.N;
    g.K = l.K;
    g.epi = epi;
    g.resid = resid;
    g.ldr = ldr;
    g.ab_fp8 = 1;
    g.acc_scale = 1.f / a_scale;
    g.w_inv_scale = l.w8_inv;
    return launch_gemm(CN_PREC_BF16, g, s);
}

int run_enc_layer_fp8(cn_model* m, const Layer& L, float* x, int B, int Tp, hipStream_t s) {
    const int d = m->cfg.d_model, M = B * Tp;
    void* q8 = m->xn;    // [M][d] e4m3fn (the bf16 buffer is twice as large)
    void* h8 = m->hbuf;  // [M][d_ff] e4m3fn
    {
        ProfScope ps(m, "layernorm_fp8", 0, (double)M * d * 5, s);
        CN_TRY(launch_layernorm_fp8(x, L.n[0].a, L.n[0].b, q8, M, d, 1e-6f, FP8_S_LN, s));
    }
    CN_TRY(run_linear_fp8(m, "qkv_proj_fp8", L.qkv, q8, FP8_S_LN, m->qkv, 3 * d, 0, 0, 1.f, M, 0, nullptr, 0, s));
    CN_TRY(run_self_attn_core(m, B, Tp, m->keymask, nullptr, 0, s));
    {
        ProfScope ps(m, "quantize_fp8", 0, (double)M * d * 3, s);
        CN_TRY(launch_quantize_fp8(m->ctx, d, q8, M, d, FP8_S_CTX, s));
    }
    CN_TRY(run_linear_fp8(m, "out_proj_fp8", L.self_o, q8, FP8_S_CTX, x, d, 1, 0, 1.f, M, CN_EPI_RESID, x, d, s));
    {
        ProfScope ps(m, "layernorm_fp8", 0, (double)M * d * 5, s);
        CN_TRY(launch_layernorm_fp8(x, L.n[1].a, L.n[1].b, q8, M, d, 1e-6f, FP8_S_LN, s));
    }
    CN_TRY(run_linear_fp8(m, "ffn_w1_fp8", L.w1, q8, FP8_S_LN, h8, L.w1.N, 0, 1, FP8_S_HID, M, CN_EPI_RELU, nullptr, 0, s));
    CN_TRY(run_linear_fp8(m, "ffn_w2_fp8", L.w2, h8, FP8_S_HID, x, d, 1, 0, 1.f, M, CN_EPI_RESID, x, d, s));
    return 0;
}

// ---- conformer sublayers (fanat_conformer_blocks.py, conformer_related.py, attention.py:68-147) ------------------
// x += scale * W2 . swish(W1 . LN(x) + b1) + ...   (SublayerConnection with the Swish feed-forward, scale 0.5 in the macaron halves)
int run_ffn_swish(cn_model* m, const Linear& w1, const Linear& w2, const Norm& n, float* x, int M, float scale, hipStream_t s) {
    const int d = m->cfg.d_model;
    CN_TRY(run_ln(m, n, x, m->xn, M, s));
    CN_TRY(run_linear(m, "ffn_w1_swish", w1, m->xn, d, m->hbuf, w1.N, 0, M, CN_EPI_SWISH, nullptr, 0, s));
    ProfScope ps(m, "ffn_w2_resid", 2.0 * M * w2.N * w2.K, (double)M * w2.K * m->es + (double)w2.N * w2.K * m->es + (double)M * w2.N * 8, s);
    GemmArgs g;
    g.A = m->hbuf;
    g.lda = w1.N;
    g.W = w2.W;
    g.bias = w2.b;
    g.C = x;
    g.ldc = d;
    g.c_f32 = 1;
    g.M = M;
    g.N = w2.N;
    g.K = w2.K;
    g.epi = CN_EPI_RESID;
    g.resid = x;
    g.ldr = d;
    g.resid_scale = scale;
    return launch_gemm(m->prec, g, s);
}

// x += O(RelAttn(LN(x))) with relative-position scores
// ctx <- relative-position attention on the fused [M][3d] projection buffer m->qkv
static int run_rel_attn_core(cn_model* m, const Layer& L, int B, int Lseq, const unsigned char* keymask, const int* klen, hipStream_t s);

int run_rel_self_attn(cn_model* m, const Layer& L, const Norm& n, float* x, int B, int Lseq, const unsigned char* keymask,
                      const int* klen, hipStream_t s) {
    const int d = m->cfg.d_model, M = B * Lseq;
    CN_TRY(run_ln(m, n, x, m->xn, M, s));
    CN_TRY(run_linear(m, "qkv_proj", L.qkv, m->xn, d, m->qkv, 3 * d, 0, M, 0, nullptr, 0, s));
    CN_TRY(run_rel_attn_core(m, L, B, Lseq, keymask, klen, s));
    return run_linear(m, "out_proj_resid", L.self_o, m->ctx, d, x, d, 1, M, CN_EPI_RESID, x, d, s);
}

static int run_rel_attn_core(cn_model* m, const Layer& L, int B, int Lseq, const unsigned char* keymask, const int* klen, hipStream_t s) {
    const int d = m->cfg.d_model, M = B * Lseq;
    AttnArgs a;
    const size_t es = m->es;
    a.Q = m->qkv;
    a.K = (const unsigned char*)m->qkv + (size_t)d * es;
    a.V = (const unsigned char*)m->qkv + (size_t)2 * d * es;
    m->ctx_blocked = false;  // (the relative-position kernel writes row-major)
    a.O = m->ctx;
    a.ldq = a.ldk = a.ldv = 3 * d;
    a.ldo = d;
    a.B = B;
    a.H = m->cfg.n_head;
    a.Lq = a.Lk = Lseq;
    a.keymask = keymask;
    a.klen = klen;
    a.scale = 1.0f / sqrtf((float)(d / m->cfg.n_head));
    a.rel_pos = L.pos_proj;
    a.rel_u = L.pos_u;
    a.rel_v = L.pos_v;
    a.rel_R = L.rel_R;
    a.ld_pos = d;
    ProfScope ps(m, "rel_self_attention", 4.0 * B * a.H * (double)Lseq * Lseq * 64, (double)M * 4 * d * m->es, s);
    return launch_attention(m->prec, a, s);
}

// x += ConvModule(LN(x))
int run_conv_module(cn_model* m, const Layer& L, const Norm& n, float* x, int B, int Lseq, hipStream_t s) {
    const int d = m->cfg.d_model, M = B * Lseq;
    CN_TRY(run_ln(m, n, x, m->xn, M, s));
    CN_TRY(run_linear(m, "conv_pointwise1", L.conv.pw1, m->xn, d, m->cv_a, 2 * d, 0, M, 0, nullptr, 0, s));
    {
        ProfScope ps(m, "conv_glu_depthwise_norm", 2.0 * M * d * L.conv.k, (double)M * d * (4 * m->es + 12), s);
        CN_TRY(launch_glu(m->prec, m->cv_a, m->xn, M, d, s));
        CN_TRY(launch_dwconv(m->prec, m->xn, L.conv.dw_w, L.conv.dw_b, m->cv_f, B, Lseq, d, L.conv.k, 0, s));
        CN_TRY(launch_groupnorm_swish(m->prec, m->cv_f, m->gn_stats, L.conv.gn_w, L.conv.gn_b, m->xn, B, Lseq, d, 1e-5f, s));
    }
    return run_linear(m, "conv_pointwise2_resid", L.conv.pw2, m->xn, d, x, d, 1, M, CN_EPI_RESID, x, d, s);
}

// SelfAttLayer, relative branch (fanat_conformer_blocks.py:26-38): ff1 (0.5), attention, convolution, ff2 (0.5)
int run_conformer_self_layer(cn_model* m, const Layer& L, float* x, int B, int Lseq, const unsigned char* keymask,
                             const int* klen, hipStream_t s) {
    const int M = B * Lseq;
    CN_TRY(run_ffn_swish(m, L.w1, L.w2, L.n[0], x, M, 0.5f, s));
    CN_TRY(run_rel_self_attn(m, L, L.n[2], x, B, Lseq, keymask, klen, s));
    CN_TRY(run_conv_module(m, L, L.n[1], x, B, Lseq, s));
    return run_ffn_swish(m, L.ff2_w1, L.ff2_w2, L.n[3], x, M, 0.5f, s);
}

// A conformer layer on the row-chain kernel (chains packed by conf_layer_chains in weights.hip): A -> relative-position
// attention -> B -> GLU / depthwise conv / GroupNorm + Swish -> C [-> source attention -> D for a mixed-attention layer].
// x_in / x_out: CHX_* layout bits of the residual stream at the layer's ends (blocked between its own launches unless
// `rowmajor`); `final_out`: where the norm packed behind the last chain goes (null: none packed).
int run_conformer_layer_chain(cn_model* m, const Layer& L, float* x, int B, int Lseq, const unsigned char* keymask, const int* klen,
                              bool mixed, int Tp, const int* src_intervals, bool rowmajor, int x_in, int x_out, void* final_out,
                              hipStream_t s) {
    const int d = m->cfg.d_model, M = B * Lseq;
    const int mid_in = rowmajor ? 0 : CHX_IN_BLK, mid_out = rowmajor ? 0 : CHX_OUT_BLK;
    CN_TRY(run_chain(m, L.cf_a, x, M, m->qkv, 3 * d, true, x_in | mid_out, s));
    CN_TRY(run_rel_attn_core(m, L, B, Lseq, keymask, klen, s));
    CN_TRY(run_chain(m, L.cf_b, x, M, m->cv_a, 2 * d, true, mid_in | mid_out, s));
    {
        ProfScope ps(m, "conv_glu_depthwise_norm", 2.0 * M * d * L.conv.k, (double)M * d * (4 * m->es + 12), s);
        CN_TRY(launch_glu(m->prec, m->cv_a, m->xn, M, d, s));
        CN_TRY(launch_dwconv(m->prec, m->xn, L.conv.dw_w, L.conv.dw_b, m->cv_f, B, Lseq, d, L.conv.k, 0, s));
        // (the module's output goes to m->ctx: the next chain's output projection is pointwise conv 2)
        CN_TRY(launch_groupnorm_swish(m->prec, m->cv_f, m->gn_stats, L.conv.gn_w, L.conv.gn_b, m->ctx, B, Lseq, d, 1e-5f, s));
        m->ctx_blocked = false;  // (row-major)
    }
    if (!mixed) return run_chain(m, L.cf_c, x, M, final_out, d, final_out != nullptr, mid_in | x_out, s);
    CN_TRY(run_chain(m, L.cf_c, x, M, m->qd, d, true, mid_in | mid_out, s));
    CN_TRY(run_src_attn_core(m, L, B, Lseq, Tp, src_intervals, s));
    return run_chain(m, L.cf_d, x, M, final_out, d, final_out != nullptr, mid_in | x_out, s);
}

// ctx <- Attn(m->qd, enc_h Wk, enc_h Wv) with the padding mask and (optionally) trigger intervals
int run_src_attn_core(cn_model* m, const Layer& L, int B, int U, int Tp, const int* intervals, hipStream_t s, bool q_blocked,
                      const int* row_off) {
    const int d = m->cfg.d_model;
    // (B counts query sets: dec_group of them share the keys / values of one utterance)
    AttnArgs a;
    if (m->kv_ready && L.kv_slot >= 0) {  // projected by the last encoder chain launch
        a.K = (const unsigned char*)m->kv_all + (size_t)L.kv_slot * 2 * d * m->es;
        a.ldk = a.ldv = m->kv_cols;
        if (m->kv_blocked) {  // ... into a blocked [M][kv_cols] matrix
            a.K = m->kv_all;
            a.kv_blocked = 1;
            a.k_col = L.kv_slot * 2 * d;
            a.v_col = a.k_col + d;
            a.kv_n = m->kv_cols;
        }
    } else {
        CN_TRY(run_linear(m, "src_kv_proj", L.src_kv, m->enc_h, d, m->kvm, 2 * d, 0, m->B * Tp, 0, nullptr, 0, s));
        a.K = m->kvm;
        a.ldk = a.ldv = 2 * d;
    }
    a.V = a.kv_blocked ? a.K : (const unsigned char*)a.K + (size_t)d * m->es;
    a.kv_mod = m->dec_group > 1 ? m->B : 0;
    a.Q = m->qd;
    if (q_blocked) {
        a.q_blocked = 1;
        a.q_col = 0;
        a.q_n = d;
        a.o_blocked = 1;
    }
    m->ctx_blocked = a.o_blocked != 0;
    a.O = m->ctx;
    a.ldq = d;
    a.ldo = d;
    a.B = B;
    a.H = m->cfg.n_head;
    a.Lq = U;
    a.Lk = Tp;
    a.keymask = m->keymask;
    if (m->ragged) {
        a.kcap = &m->utt_meta[0].tp;
        a.kcap_stride = (int)(sizeof(UttMeta) / sizeof(int));
    }
    a.intervals = intervals;
    a.iv_stride = Tp + 1;
    a.row_off = row_off;  // (packed query rows; the keys are encoder frames either way)
    a.scale = 1.0f / sqrtf((float)(d / m->cfg.n_head));
    ProfScope ps(m, "src_attention", 4.0 * B * a.H * (double)U * Tp * 64,
                 ((double)B * U * 2 * d + (double)B * Tp * 2 * d) * m->es, s);
    return launch_attention(m->prec, a, s);
}

// x += O(Attn(LN(x) Wq, mem Wk, mem Wv))
int run_src_attn(cn_model* m, const Layer& L, const Norm* pre, float* x, int B, int U, int Tp, const int* intervals,
                 hipStream_t s) {
    const int d = m->cfg.d_model;
    if (pre) CN_TRY(run_ln(m, *pre, x, m->xn, B * U, s));
    CN_TRY(run_linear(m, "src_q_proj", L.src_q, m->xn, d, m->qd, d, 0, B * U, 0, nullptr, 0, s));
    CN_TRY(run_src_attn_core(m, L, B, U, Tp, intervals, s));
    CN_TRY(run_linear(m, "out_proj_resid", L.src_o, m->ctx, d, x, d, 1, B * U, CN_EPI_RESID, x, d, s));
    return 0;
}

// generator tail: argmax + max log-prob per row.  Fused kernel (no logits tensor) unless full rows are needed.
int run_generator(cn_model* m, const Linear& g, const void* h, int M, int* arg, float* maxlp, bool need_rows,
                  hipStream_t s, const int* m_dev) {
    const int d = m->cfg.d_model, V = m->cfg.vocab_size;
    if (g.gm_w && !need_rows) {
        const bool x3 = m->prec == CN_PREC_X3;
        ProfScope ps(m, "generator_argmax_fused", (x3 ? 6.0 : 2.0) * M * V * d, ((double)M * d + (double)V * d) * (x3 ? 4 : 2), s);
        GenmaxArgs a;
        a.x3 = x3;
        a.h = h;
        a.wp = g.gm_w;
        a.bp = g.gm_b;
        a.arg = arg;
        a.maxlp = maxlp;
        a.M = M;
        a.m_dev = m_dev;
        a.V = V;
        a.d = d;
        return launch_genmax(a, s);
    }
    // the logits buffer holds B x (T' + 1) rows (one alignment per utterance); the decoder side of an ESA group brings G times
    // that: the rows go through it in chunks (the engines without the fused kernel - fp32, bf16x3 - wrote past the buffer here)
    const size_t cap_rows = (size_t)m->maxB * (m->maxTp + 1);
    if ((size_t)M > cap_rows && need_rows) {
        cn_set_error("generator: full log-probability rows (capture / beam_width > 1) of more rows than one alignment per utterance");
        return -1;
    }
    for (size_t r0 = 0; r0 < (size_t)M; r0 += cap_rows) {
        const int rows = (int)std::min(cap_rows, (size_t)M - r0);
        CN_TRY(run_linear(m, "generator_proj", g, (const unsigned char*)h + r0 * d * m->es, d, m->logits, V, 1, rows, 0, nullptr, 0, s));
        ProfScope ps(m, "logsoftmax_argmax", 0, (double)rows * V * 4, s);
        CN_TRY(launch_logsoftmax_argmax(m->logits, rows, V, V, arg + r0, maxlp ? maxlp + r0 : nullptr, need_rows ? 1 : 0, s));
    }
    return 0;
}

}  // namespace cn_host
