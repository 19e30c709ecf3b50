// Private to the translation units that take a model handle (handle.hip, weights.hip, workspace.hip, sublayers.hip,
// model.hip, decode_ar.hip): the handle behind the opaque cn_model of include/cassnat_hip.h, the structs it is made of,
// and the internal functions that cross those files.  No kernel file includes it.  Everything but cn_model itself (a global
// tag: the public header forward-declares it) lives in namespace cn_host.  (CN_TRY: common.h)
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cassnat_hip.h"
#include "../../include/cassnat_hip_ctc_bias.h"
#include "kernels.h"

namespace cn_host {

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

struct Linear {
    void* W = nullptr;  // [N][K] model precision
    float* b = nullptr;
    int N = 0, K = 0;
    void* W8 = nullptr;          // fp8 encoder mode (config 5): e4m3fn copy [N][K] at a per-tensor power-of-two scale ...
    float* w8_inv = nullptr;     // ... and 1 / scale (one float in the blob: it travels with a weight broadcast)
    void* px3 = nullptr;    // split-bf16 engine, K == 256: pack_proj_x3 fragment stream (proj_x3.hip)
    void* gm_w = nullptr;   // generators only (bf16, d_model 256): pack_genmax fragment stream ...
    float* gm_b = nullptr;  // ... and padded biases for the fused argmax kernel
};
struct Norm {
    float* a = nullptr;
    float* b = nullptr;
};
// conformer convolution module (conformer_related.py:15-44)
struct ConvMod {
    Linear pw1, pw2;            // pointwise convs as [2d][d] / [d][d] matrices
    float *dw_w = nullptr, *dw_b = nullptr;  // depthwise [d][k] fp32, bias [d]
    float *gn_w = nullptr, *gn_b = nullptr;  // GroupNorm(1, d) affine
    int k = 0;
};
// fp8 engine: scale of the e4m3 image conv1 writes for conv2's e4m3 form (ReLU outputs: x8, saturating at 56 - as the hidden
// activations of the feed-forward products)
constexpr float FP8_S_IMG = 8.f;
struct ChainRef {
    void* w = nullptr;
    float* tab = nullptr;
    int dff = 0, tail_n = 0;
    bool has_wo = false, has_next = false, swish = false;
    int* f8q = nullptr;  // e4m3 feed-forward units (chain.hip, F8 form): the four scale bytes of its products, in the blob
};
struct Layer {
    Norm n[5];
    // conformer blocks: w1/w2 are feed_forward1 (or the extractor's feed_forward), ff2_* feed_forward2; relative-position
    // self attention keeps the projected position rows P = table . W_pos^T [(2R+1)][d] and the biases u, v [d] in fp32
    Linear ff2_w1, ff2_w2;
    ConvMod conv;
    float *pos_proj = nullptr, *pos_u = nullptr, *pos_v = nullptr;
    int rel_R = 0;
    bool conformer = false;
    ChainRef cf_a, cf_b, cf_c, cf_d;  // conformer layer on the row-chain kernel (bf16 / d_model 256): see conf_layer_chains
    int kv_slot = -1;  // >= 0: this layer's cross-attention K|V are columns kv_slot * 2d.. of m->kv_all (written by the last encoder chain)
    Linear qkv;       // self-attention: fused Q|K|V projection
    Linear self_o;
    Linear src_q, src_kv, src_o;  // source attention: Q from the stream, K|V from the encoder memory
    Linear w1, w2;
    void *w1p = nullptr, *w2p = nullptr;  // fused-FFN fragment streams (bf16, d_model == 256); then w1/w2 hold biases only
    void* wx3 = nullptr;  // split-bf16 engine: the fused-FFN stream of fused_x3.hip (hi and lo fragments); w1/w2 hold biases only
    bool ff_swish = false;  // feed_forward's hidden activation is Swish, residual scale 1 (the conformer AST's decoder layers) - else ReLU
    bool has_self = false, has_src = false;
};

// One packed stream of the row-chain kernel (chain.hip): [attention output projection] + [FFN] + [the NEXT sublayer's
// pre-norm and input projection: tail_n columns, 0 = the norm itself is the output]
// decoder-side sublayers in execution order (extractor: src; SAD: self; MAD: self, src), each followed by its chain
struct DecStep {
    int stack = 0;       // 0 extractor, 1 SAD, 2 MAD
    int layer = 0;
    bool self = false;   // self attention (else source attention)
    ChainRef chain;      // after this sublayer's attention
    ChainRef entry;      // pre-norm + input projection alone (first step; first MAD step when use_unimask shifts the stream)
};

struct ProfPending {
    const char* tag;
    hipEvent_t a, b;
    double flops, bytes;
};
struct ProfStat {
    long long count = 0;
    double ms = 0, flops = 0, bytes = 0;
};

struct Capture {
    void* p = nullptr;
    size_t bytes = 0;
    int dtype = CN_DTYPE_F32;
    std::vector<int64_t> shape;
    long long call = -1;  // the engine call (cn_model::call_id) that produced it
};

}  // namespace cn_host

struct cn_model {
    cn_config cfg;
    int prec = 0;
    int fp8_scope = 0;     // CN_FP8_* bits in force (cn_config.fp8_scope, 0 resolved to all)
    bool fp8_enc = false;  // CN_PRECISION_FP8: bf16 engine whose encoder-layer products run on the fp8 MFMA (BASELINE config 5)
    size_t es = 4;
    std::map<std::string, cn_host::HostTensor> host;
    std::vector<float> pe_host;
    int pe_rows = 0;
    bool finalized = false;

    // packed weights: owned through a reference count, so that several handles (the decode pipelines of one GPU, or a
    // handle rebuilt for a larger workspace) use ONE device copy (cn_model_create_shared)
    struct BlobOwner {
        unsigned char* p = nullptr;
        ~BlobOwner() {
            if (p) (void)hipFree(p);
        }
    };
    std::shared_ptr<BlobOwner> blob_owner;
    bool blob_borrowed = false;  // the blob belongs to a donor handle: never re-packed or re-allocated here
    unsigned char* blob = nullptr;
    size_t blob_bytes = 0;

    // weight views into the blob
    float* conv1_w = nullptr;  // [9][C]
    float* conv1_b = nullptr;
    cn_host::Linear conv2;       // [C][9C] (kh,kw,cin)
    void* conv2_f8w = nullptr;  // fp8 engine, 256 channels: the same matrix as e4m3fn bytes at a per-tensor power-of-two scale, and
    int* conv2_f8q = nullptr;   // the two E8M0 scale bytes of conv2.hip's e4m3 form {127 - log2(weight scale), 127 - log2(image scale)}
    void* linear_f8w = nullptr;  // fp8 engine: linear_out's (column-permuted) matrix as e4m3fn bytes, and its two scale bytes
    int* linear_f8q = nullptr;   // {127 - log2(weight scale), 127 - log2(scale of conv2's e4m3 output)}
    void* conv2_x3w = nullptr;  // split-bf16 engine, 256 channels: the same matrix as two bf16 planes (hi, then lo) for conv2.hip's X3 form
    // ... and for conv2.hip's MIX form (half-precision hi x hi + e4m3 cross terms: 2 MFMA units per product instead of 3): the
    // half-precision matrix, then the q = e4m3(w S_q) and l = e4m3((w - hi) S_l) bytes; conv2_mixq = the four E8M0 scale bytes
    void* conv2_mixw = nullptr;
    int* conv2_mixq = nullptr;
    cn_host::Linear linear_out;  // [d][F2*C] (f,c)
    std::vector<cn_host::Layer> enc, extra, sad, mad;
    std::vector<cn_host::ChainRef> enc_chain;  // one per encoder layer when the row-chain path applies, else empty
    cn_host::ChainRef enc_entry;               // LayerNorm + Q|K|V projection of encoder layer 0 (the rows come from linear_out)
    std::vector<cn_host::DecStep> dec_steps;   // decoder-side sublayers with their chains when the path applies, else empty
    cn_host::Norm enc_norm, dec_norm;
    cn_host::Linear ctc_gen, att_gen;
    float* pe = nullptr;  // [pe_rows][d]

    // geometry of the workspace
    int maxB = 0, maxT = 0, maxT1 = 0, maxTp = 0, F1 = 0, F2 = 0;
    int maxU = 0;  // utterances a call may carry at most (buffers with one entry per utterance are sized for it): a merged pass
                   // of short utterances fits more of them than max_batch into the workspace's max_batch x max_frames area
    std::vector<void*> allocs;
    std::map<std::string, size_t> ws_cap;  // bytes allocated per workspace buffer: every call is checked against it (ws_check)
    // merged engine pass (cn_decode_nast_merged): per-utterance records of the reference batches it carries
    UttMeta* utt_meta = nullptr;
    int* row_off = nullptr;    // [utterances + 1] packed decoder rows of the current pass (launch_row_plan); row_off[B] = their total
    bool rows_packed = false;  // the last decoder pass ran on them (tok / val are then not [B][U])
    bool ragged = false;       // the current call has them
    bool ragged_next = false;  // set by cn_decode_nast_merged right before its encoder stage
    bool u_predicted = false;  // the current call's decoder side runs on a predicted row count (>= the true one, or the ticket says so)
    // row-count prediction (cn_decode_nast_merged, u_hint): the decoder side ran on `ticket_U` rows before the true count was
    // known; the count lands in one of four page-locked words (a ticket names its word) for cn_decode_ticket
    int* ymax_ring = nullptr;  // [4], page-locked
    int ticket_U[4] = {0, 0, 0, 0};
    int ticket_id[4] = {-1, -1, -1, -1};  // the ticket (sequence number) whose pass owns the word now: an older ticket has expired
    long long ticket_seq = 0;
    unsigned char* keymask = nullptr;
    void *c1 = nullptr, *c2 = nullptr;
    float* x = nullptr;
    void *xn = nullptr, *qkv = nullptr, *ctx = nullptr, *hbuf = nullptr, *enc_h = nullptr, *kvm = nullptr, *qd = nullptr,
         *dec_h = nullptr;
    float *xd = nullptr, *xd2 = nullptr, *logits = nullptr;
    int *best = nullptr, *shift = nullptr, *src_size = nullptr, *ylen = nullptr, *ymax = nullptr, *intervals = nullptr,
        *tok = nullptr, *topk_idx = nullptr;
    float *ctc_maxlp = nullptr, *val = nullptr, *topk_val = nullptr;
    void* kv_all = nullptr;   // [M][kv_cols] bf16: cross-attention K|V of every decoder-side layer, projected by the last encoder
    int kv_cols = 0;          // chain launch's tail (0: each layer projects its own into kvm)
    bool kv_ready = false;    // ... and that launch ran for the current batch
    bool kv_blocked = false;  // ... writing the blocked layout (common.h: cn_blk16_off)
    bool ctx_blocked = false; // m->ctx holds the attention kernel's o_blocked form (its reader is the row-chain kernel)
    long long call_id = 0;  // counts encoder passes: a captured tensor is only served for the call that wrote it
    int c1_halo_B = -1, c1_halo_T1 = -1;  // shape of the haloed conv1 image the buffer currently holds (-1: none)
    bool ctc_maxlp_valid = false;  // the fused arg-max-only CTC generator does not produce it

    void* cv_a = nullptr;      // conformer convolution module scratch
    float* cv_f = nullptr;
    double* gn_stats = nullptr;
    int* ymax_pinned = nullptr;  // page-locked host word for the one data-dependent readback per batch
    // fp16 build (CN_OP16_F16): half-precision operands have a range.  What drives magnitudes from outside is the scale of the
    // features (everything behind linear_out is LayerNorm-ed in fp32 first), so every pass checks them against the largest value
    // for which neither subsampling convolution's output can leave the half range (op16_feat_limit: a word of the weight blob,
    // from the convolutions' weight row sums) and raises a sticky flag in device-visible page-locked memory (cn_take_range_fault).
    // The other build uses the same guard for its split-bf16 engines: conv1's outputs against the e4m3 range of conv2's MIX form
    const float* op16_feat_limit = nullptr;
    float op16_feat_limit_host = -1.f;  // (read back once, on the first cn_take_range_fault)
    unsigned int* op16_fault = nullptr;
    // CTC prefix beam / forced alignment scratch (cn_ctc_beam, cn_decode_nast_forced): grown on demand
    std::map<std::string, std::pair<void*, size_t>> scratch;

    // autoregressive (AST) decoder state (cn_ast_*): token embedding, per-layer cross K|V, KV cache, CTC prefix states
    float* tgt_lut = nullptr;  // [V][d] fp32 (view into the blob)
    int ast_max_len = 0, ast_slots = 0, ast_ctc_beam = 0, ast_Tp_cap = 0, ast_blank = 0;
    std::vector<void*> ast_kvx, ast_ck, ast_cv;  // per decoder layer
    float *ast_logits = nullptr, *ast_r0 = nullptr, *ast_r[2] = {nullptr, nullptr}, *ast_maxlp = nullptr;
    int* ast_arg = nullptr;
    std::vector<void*> ast_allocs;
    AstBeamState beam;  // device-side beam search state (cn_decode_ast)
    int beam_S = 0, beam_L = 0, beam_K = 0;
    int *beam_idx = nullptr;
    float *beam_val = nullptr, *beam_ctc = nullptr, *beam_lm = nullptr;
    // LM shallow fusion (cn_ast_attach_lm; cn_nat_attach_lm on a CASS-NAT handle, whose finish loop steps it): the TransformerLM
    // handle whose step runs beside this decoder's.  On an LM handle
    // (cfg.ast = 2) the ast_ck / ast_cv / ast_logits fields above hold ITS step cache [layer][pos][slot][d] and logits.
    cn_model* ast_lm = nullptr;
    // word n-gram shallow fusion (cn_ast_attach_ngram; cn_nat_attach_ngram on a CASS-NAT handle): the desc by value (device tables the caller keeps alive), lm_weight * ln 10
    // as float32, and the per-slot (a_word, a_eos) pairs of cn_decode_ast's step loop
    cn_ngram_desc ast_ng = {};
    bool ast_ng_on = false;
    float ast_ng_scale = 0.f;
    float* beam_adds = nullptr;  // [S][2]
    // contextual phrase biasing (cn_ast_attach_bias): the desc by value (device tables the caller keeps alive) and the nodes of
    // cn_decode_ast's beam slots at the last two positions
    cn_bias_desc ast_bias = {};
    bool ast_bias_on = false;
    int32_t* beam_node[2] = {nullptr, nullptr};  // [S] each
    const void* lib_tag = nullptr;  // which of the two libraries created the handle (an attach never crosses them)

    // last call
    int B = 0, T = 0, T1 = 0, Tp = 0, U = 0, last_k = 0;
    int att_rows_U = 0;  // > 0: m->logits holds the decoder's log-probability rows [B][att_rows_U][V] of the last pass (cn_nat_lm_finish)
    int dec_group = 1;  // decoder-side batch = B * dec_group (ESA: that many alignments per utterance in one pass), else 1
    std::map<std::string, cn_host::Capture> captures;

    // per-kernel-tag timing with HIP events on the launch stream (cn_profile_begin / cn_profile_end)
    bool prof_on = false;
    std::string prof_filter;  // empty: every tag
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<cn_host::ProfPending> prof_pending;
    std::map<std::string, cn_host::ProfStat> prof_stats;
};

namespace cn_host {

// Brackets the launches of one kernel tag with two events on the stream when profiling is on.
struct ProfScope {
    cn_model* m;
    hipStream_t s;
    ProfPending pp;
    bool live = false;
    ProfScope(cn_model* m_, const char* tag, double flops, double bytes, hipStream_t s_) : m(m_), s(s_) {
        if (!m->prof_on) return;
        if (!m->prof_filter.empty() && m->prof_filter.find(std::string("|") + tag + "|") == std::string::npos) return;
        while (m->ev_pool.size() < m->ev_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            m->ev_pool.push_back(e);
        }
        pp.tag = tag;
        pp.a = m->ev_pool[m->ev_used++];
        pp.b = m->ev_pool[m->ev_used++];
        pp.flops = flops;
        pp.bytes = bytes;
        live = hipEventRecord(pp.a, s) == hipSuccess;
    }
    ~ProfScope() {
        if (live && hipEventRecord(pp.b, s) == hipSuccess) m->prof_pending.push_back(pp);
    }
};

// ---- weights.hip ----
// Packs the loaded tensors into the weight blob (or lays the views over a borrowed / broadcast one) and fills every weight
// view of the handle
int build_weights(cn_model* m);

// ---- workspace.hip ----
int build_workspace(cn_model* m);
// Every buffer of the workspace against what a call of (B utterances, T frames, G alignments per utterance) needs
int ws_check(cn_model* m, int B, int T, int G, const char* what);
// Copy of a device tensor kept for cn_fetch (cn_decode_opts.capture)
int capture(cn_model* m, const char* name, const void* src, bool model_prec, int dtype, std::vector<int64_t> shape, hipStream_t s);
// Named device scratch of the handle, grown on demand
int scratch_buf(cn_model* m, const char* name, size_t bytes, void** out);

// ---- sublayers.hip: the building blocks of every pipeline ----
int run_linear(cn_model* m, const char* tag, const Linear& l, const void* A, int lda, void* C, int ldc, int c_f32, int M, int epi,
               const float* resid, int ldr, hipStream_t s);
int run_ln(cn_model* m, const Norm& n, const float* x, void* y, int M, hipStream_t s);
int run_ffn(cn_model* m, const Layer& L, const Norm& n, float* x, int M, const Norm* next, void* next_out, hipStream_t s);
bool x3_chain_applies(const cn_model* m, const Layer& L, const Linear* tail);
int run_x3_chain(cn_model* m, const Layer& L, const Norm& n1, float* x, int M, const Norm& next, void* next_out, const Linear* tail,
                 void* tail_out, int ld_tail, const char* tag, hipStream_t s);
int run_self_attn_core(cn_model* m, int B, int Lseq, const unsigned char* keymask, const int* klen, int causal, hipStream_t s,
                       bool blocked = false, const int* row_off = nullptr, const ChainRef* proj = nullptr);
int run_self_attn(cn_model* m, const Layer& L, const Norm* pre, float* x, int B, int Lseq, const unsigned char* keymask,
                  const int* klen, int causal, hipStream_t s);
// x_mode of run_chain: the fp32 stream is read / written row-major or in the kernel's blocked tile layout, or not written
enum { CHX_IN_BLK = 1, CHX_OUT_BLK = 2, CHX_NO_STORE = 4 };
int run_chain(cn_model* m, const ChainRef& r, float* x, int M, void* out, int ldo, bool with_next, int x_mode, hipStream_t s,
              void* ln_out = nullptr, int ld_ln = 0, bool out_blocked = false, const char* tag = "row_chain",
              const int* m_dev = nullptr, bool ln_only = false);
int run_enc_layer_fp8(cn_model* m, const Layer& L, float* x, int B, int Tp, hipStream_t s);
int run_ffn_swish(cn_model* m, const Linear& w1, const Linear& w2, const Norm& n, float* x, int M, float scale, hipStream_t s);
int run_rel_self_attn(cn_model* m, const Layer& L, const Norm& n, float* x, int B, int Lseq, const unsigned char* keymask,
                      const int* klen, hipStream_t s);
int run_conv_module(cn_model* m, const Layer& L, const Norm& n, float* x, int B, int Lseq, hipStream_t s);
int run_conformer_self_layer(cn_model* m, const Layer& L, float* x, int B, int Lseq, const unsigned char* keymask, const int* klen,
                             hipStream_t s);
int run_conformer_layer_chain(cn_model* m, const Layer& L, float* x, int B, int Lseq, const unsigned char* keymask, const int* klen,
                              bool mixed, int Tp, const int* src_intervals, bool rowmajor, int x_in, int x_out, void* final_out,
                              hipStream_t s);
int run_src_attn_core(cn_model* m, const Layer& L, int B, int U, int Tp, const int* intervals, hipStream_t s, bool q_blocked = false,
                      const int* row_off = nullptr);
int run_src_attn(cn_model* m, const Layer& L, const Norm* pre, float* x, int B, int U, int Tp, const int* intervals, hipStream_t s);
int run_generator(cn_model* m, const Linear& g, const void* h, int M, int* arg, float* maxlp, bool need_rows, hipStream_t s,
                  const int* m_dev = nullptr);

// ---- model.hip: the NAT stages ----
int check_call(cn_model* m, int B, int T, int F, bool area = false);
int stage_encode(cn_model* m, const float* feats, int B, int T, int F, const cn_decode_opts* o, hipStream_t s);
int stage_encode_ctc_rows(cn_model* m, const float* feats, int B, int T, int F, const cn_decode_opts* o, hipStream_t s);

// ---- decode_ar.hip: the TransformerLM's step, also run by the NAT finish loop and the CTC + LM beam ----
int lm_prepare_buffers(cn_model* lm, int max_len, int max_slots);
int lm_check_step(const cn_model* lm, int max_len, int max_slots, const char* who);
int lm_check_pair(const cn_model* m, const cn_model* lm, const char* who);
int lm_step_run(cn_model* lm, int n, int pos, const int32_t* tok_dev, const int32_t* anc_dev, const uint8_t* keyok_dev,
                int table_stride, hipStream_t s, const int32_t* row_pos = nullptr, const int32_t* row_stay = nullptr);

}  // namespace cn_host
