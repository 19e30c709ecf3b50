// C-ABI of libcassnat_hip.so, the model handle: the error string and version, create / load / finalize / destroy, the weight-blob
// hand-off, the range-guard flag, the per-tag profiler and cn_fetch.  The weight packer is weights.hip, the workspace
// workspace.hip, the decode paths model.hip and decode_ar.hip.  See include/cassnat_hip.h for the contract.
#include <cstdio>
#include <cstring>

#include "model.h"

using namespace cn_host;

static thread_local std::string g_last_error;
static const int g_lib_tag = 0;  // its address tells this library's handles from the other build's
void cn_set_error(const std::string& msg) { g_last_error = msg; }
extern "C" const char* cn_last_error(void) { return g_last_error.c_str(); }
extern "C" const char* cn_version(void) { return "cassnat_hip 0.1 (gfx950, 16-bit operand " CN_OP16_NAME ")"; }
extern "C" const char* cn_operand16(void) { return CN_OP16_NAME; }

// The library exists in two builds that differ in the 16-bit MFMA operand (common.h): this one's engines of the 16-bit kind are
// CN_PRECISION_BF16 (+ FP8, BF16X3, F32) - or, built with -DCN_OP16_F16, CN_PRECISION_F16 and nothing else.  Returns the internal
// precision of a request, -1 (error set) when it belongs to the other build.
int cn_own_precision(int32_t precision, const char* who) {
#ifdef CN_OP16_F16
    if (precision == CN_PRECISION_F16) return CN_PREC_BF16;  // (the 16-bit path; its operand type is this build's)
    cn_set_error(std::string(who) + ": this build of the library (libcassnat_hip_f16.so) holds the fp16 engine only (CN_PRECISION_F16)");
    return -1;
#else
    if (precision == CN_PRECISION_F16) {
        cn_set_error(std::string(who) + ": CN_PRECISION_F16 engines live in libcassnat_hip_f16.so (the -DCN_OP16_F16 build of these sources)");
        return -1;
    }
    return precision;
#endif
}

// ---------------------------------------------------------------------------------------------
// exported functions
// ---------------------------------------------------------------------------------------------
extern "C" int cn_model_create(const cn_config* cfg, cn_model** out) {
    if (!cfg || !out) {
        cn_set_error("cn_model_create: null argument");
        return -1;
    }
    const cn_config& c = *cfg;
    if (c.d_model % 64 != 0 || c.n_head < 1 || c.d_model != 64 * c.n_head) {
        cn_set_error("cn_model_create: this build needs d_model == 64 * n_head (d_k = 64)");
        return -1;
    }
    if (c.d_encff % 64 || c.d_decff % 64 || c.d_model > 1024) {
        cn_set_error("cn_model_create: feed-forward widths must be multiples of 64 and d_model <= 1024");
        return -1;
    }
    if (c.precision != CN_PRECISION_F32 && c.precision != CN_PRECISION_BF16 && c.precision != CN_PRECISION_FP8 &&
        c.precision != CN_PRECISION_BF16X3 && c.precision != CN_PRECISION_F16) {
        cn_set_error("cn_model_create: unknown precision");
        return -1;
    }
    const int own_prec = cn_own_precision(c.precision, "cn_model_create");
    if (own_prec < 0) return -1;
    if (c.precision == CN_PRECISION_BF16X3 && (c.d_encff % 32 || c.d_decff % 32 || c.d_model % 32 || c.d_ff % 32)) {
        cn_set_error("cn_model_create: the split-bf16 (bf16x3) engine needs d_model and the feed-forward widths to be multiples of 32");
        return -1;
    }
    if (c.precision == CN_PRECISION_FP8 && (c.ast || c.conf_enc || c.d_model % 128 != 0 || c.d_encff % 128 != 0)) {
        cn_set_error("cn_model_create: the fp8 encoder mode covers the transformer-block NAT model with d_model, d_encff % 128 == 0");
        return -1;
    }
    if (c.fp8_scope < 0 || c.fp8_scope > 7 || ((c.fp8_scope & CN_FP8_LINEAR) && !(c.fp8_scope & CN_FP8_CONV2)) || c.fp8_ffn_first_layer < 0) {
        cn_set_error("cn_model_create: fp8_scope is a mask of CN_FP8_CONV2 | CN_FP8_LINEAR | CN_FP8_FFN (LINEAR needs CONV2), fp8_ffn_first_layer >= 0");
        return -1;
    }
    // cfg.ast == 1 with conf_enc = the reference's models/conformer.py (conformer encoder, transformer decoder with Swish FFNs);
    // the reference has no autoregressive model with conformer decoder blocks, and no conformer TransformerLM
    if ((c.ast == 1 && c.conf_dec) || (c.ast == 2 && (c.conf_enc || c.conf_dec))) {
        cn_set_error(c.ast == 1 ? "cn_model_create: the autoregressive model (ast = 1) has no conformer decoder (conf_dec = 1): the reference "
                                  "defines none (models/conformer.py keeps transformer decoder layers)"
                                : "cn_model_create: the TransformerLM (ast = 2) has no conformer blocks");
        return -1;
    }
    // the reference's Conv1d(padding = (k - 1) // 2) yields L - 1 frames for an even k and its residual add fails
    if (c.conf_enc && (c.enc_kernel < 1 || c.enc_kernel % 2 == 0)) {
        cn_set_error("cn_model_create: enc_kernel must be odd and >= 1 for a conformer encoder (conf_enc = 1), got " + std::to_string(c.enc_kernel));
        return -1;
    }
    if (c.conf_dec && (c.dec_kernel < 1 || c.dec_kernel % 2 == 0)) {
        cn_set_error("cn_model_create: dec_kernel must be odd and >= 1 for a conformer decoder (conf_dec = 1), got " + std::to_string(c.dec_kernel));
        return -1;
    }
    if (c.input_size < 4 || c.vocab_size < 4 || c.max_batch < 1 || c.max_frames < 4 || c.n_enc < 0 || c.n_extra < 0 ||
        c.n_self_dec < 0 || c.n_mix_dec < 0) {
        cn_set_error("cn_model_create: bad dimensions");
        return -1;
    }
    CN_HIP_CHECK(hipSetDevice(c.device));
    cn_model* m = new cn_model();
    m->cfg = c;
    m->lib_tag = &g_lib_tag;
    // fp8: a bf16 engine (storage, decoder side, conv front-end) whose encoder-layer products take e4m3fn operands
    m->fp8_enc = c.precision == CN_PRECISION_FP8;
    m->fp8_scope = c.fp8_scope ? c.fp8_scope : (CN_FP8_CONV2 | CN_FP8_LINEAR | CN_FP8_FFN);
    m->prec = m->fp8_enc ? CN_PREC_BF16 : (c.precision == CN_PRECISION_BF16X3 ? CN_PREC_X3 : own_prec);
    m->es = cn_elem_size(m->prec);
    m->maxB = c.max_batch;
    m->maxT = c.max_frames;
    m->maxT1 = (c.max_frames - 1) / 2 + 1;
    m->maxTp = (m->maxT1 - 1) / 2 + 1;
    m->maxU = 16 * c.max_batch;
    m->F1 = (c.input_size - 1) / 2 + 1;
    m->F2 = (m->F1 - 1) / 2 + 1;
    *out = m;
    return 0;
}

extern "C" int cn_model_create_shared(const cn_config* cfg, cn_model* donor, cn_model** out) {
    if (!donor || !donor->finalized || !donor->blob) {
        cn_set_error("cn_model_create_shared: the donor must be a finalized model");
        return -1;
    }
    if (cfg->device != donor->cfg.device || cfg->precision != donor->cfg.precision) {
        cn_set_error("cn_model_create_shared: device and precision must be the donor's");
        return -1;
    }
    cn_model* m = nullptr;
    CN_TRY(cn_model_create(cfg, &m));
    m->blob_owner = donor->blob_owner;
    m->blob = donor->blob;
    m->blob_bytes = donor->blob_bytes;
    m->blob_borrowed = true;
    m->pe_rows = donor->pe_rows;
    const int rc = cn_model_finalize(m);  // layout pass over the donor's blob + this handle's own workspace
    if (rc != 0) {
        cn_model_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

extern "C" void cn_model_destroy(cn_model* m) {
    if (!m) return;
    for (void* p : m->allocs) (void)hipFree(p);
    for (auto& kv : m->captures)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto e : m->ev_pool) (void)hipEventDestroy(e);
    if (m->ymax_pinned) (void)hipHostFree(m->ymax_pinned);
    if (m->ymax_ring) (void)hipHostFree(m->ymax_ring);
    if (m->op16_fault) (void)hipHostFree(m->op16_fault);
    for (void* q : m->ast_allocs) (void)hipFree(q);
    for (auto& kv : m->scratch)
        if (kv.second.first) (void)hipFree(kv.second.first);
    m->blob_owner.reset();  // the last handle that uses the blob frees it
    delete m;
}

extern "C" int cn_model_load_weights(cn_model* m, const char* name, const float* host_data, const int64_t* shape,
                                     int32_t ndim) {
    if (!m || !name || !host_data || !shape || ndim < 1 || ndim > 4) {
        cn_set_error("cn_model_load_weights: bad argument");
        return -1;
    }
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(host_data, host_data + n);
    m->host[name] = std::move(t);
    m->finalized = false;
    return 0;
}

extern "C" int cn_model_load_pe(cn_model* m, const float* host_table, int32_t rows) {
    if (!m || !host_table || rows < 1) {
        cn_set_error("cn_model_load_pe: bad argument");
        return -1;
    }
    m->pe_host.assign(host_table, host_table + (size_t)rows * m->cfg.d_model);
    m->pe_rows = rows;
    m->finalized = false;
    return 0;
}

extern "C" int cn_model_finalize(cn_model* m) {
    if (!m) {
        cn_set_error("cn_model_finalize: null model");
        return -1;
    }
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    m->op16_feat_limit_host = -1.f;  // (the range guard's bound is a word of the weights: read back again after this)
    if (m->pe_rows < m->maxTp + 1) {
        if (m->host.empty() && m->pe_rows == 0) {
            m->pe_rows = 5000;  // layout-only: table arrives with the broadcast blob (create_pe max_len)
        } else {
            cn_set_error("cn_model_finalize: positional table missing or shorter than max_frames/4 + 1");
            return -1;
        }
    }
    CN_TRY(build_weights(m));
    CN_TRY(build_workspace(m));
    m->finalized = true;
    return 0;
}

extern "C" int cn_model_weight_blob(cn_model* m, void** dev_ptr, int64_t* bytes) {
    if (!m || !m->blob) {
        cn_set_error("cn_model_weight_blob: finalize first");
        return -1;
    }
    *dev_ptr = m->blob;
    *bytes = (int64_t)m->blob_bytes;
    return 0;
}

// fp16 engines: has a pass since the last call seen features beyond the range the engine's half-precision operands hold (then
// its results are not to be used)?  Valid once the passes' stream work is done; clears the flag.  Other engines: always 0.
extern "C" int cn_take_range_fault(cn_model* m, int32_t* fault_host, float* feature_limit_host) {
    if (!m || !fault_host) {
        cn_set_error("cn_take_range_fault: bad arguments");
        return -1;
    }
    *fault_host = 0;
    if (feature_limit_host) *feature_limit_host = 0.f;
    if (!m->op16_fault) return 0;
    *fault_host = (int32_t)__atomic_exchange_n(m->op16_fault, 0u, __ATOMIC_ACQ_REL);
    if (feature_limit_host && m->op16_feat_limit) {
        if (m->op16_feat_limit_host < 0.f) CN_HIP_CHECK(hipMemcpy(&m->op16_feat_limit_host, m->op16_feat_limit, 4, hipMemcpyDeviceToHost));
        *feature_limit_host = m->op16_feat_limit_host;
    }
    return 0;
}

extern "C" int cn_profile_begin(cn_model* m, const char* tags) {
    if (!m) {
        cn_set_error("cn_profile_begin: null model");
        return -1;
    }
    m->prof_on = true;
    m->prof_filter = (tags && *tags) ? std::string("|") + tags + "|" : std::string();
    m->prof_pending.clear();
    m->prof_stats.clear();
    m->ev_used = 0;
    // events for a few thousand tagged launches exist before the caller's timed region starts (the pool still grows on
    // demand past that)
    while (m->ev_pool.size() < 4096) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) break;
        m->ev_pool.push_back(e);
    }
    return 0;
}

extern "C" int cn_profile_end(cn_model* m, char* json_out, int64_t cap) {
    if (!m) {
        cn_set_error("cn_profile_end: null model");
        return -1;
    }
    CN_HIP_CHECK(hipDeviceSynchronize());
    for (auto& pp : m->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pp.a, pp.b) != hipSuccess) continue;
        ProfStat& st = m->prof_stats[pp.tag];
        st.count += 1;
        st.ms += ms;
        st.flops += pp.flops;
        st.bytes += pp.bytes;
    }
    m->prof_pending.clear();
    m->prof_on = false;
    m->ev_used = 0;
    std::string js = "{";
    bool first = true;
    for (auto& kv : m->prof_stats) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s\"%s\": {\"count\": %lld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}",
                 first ? "" : ", ", kv.first.c_str(), kv.second.count, kv.second.ms, kv.second.flops, kv.second.bytes);
        js += buf;
        first = false;
    }
    js += "}";
    if (json_out && cap > 0) {
        if ((int64_t)js.size() + 1 > cap) {
            cn_set_error("cn_profile_end: buffer too small");
            return -1;
        }
        std::memcpy(json_out, js.c_str(), js.size() + 1);
    }
    return 0;
}

extern "C" int cn_fetch(cn_model* m, const char* name, void* host_dst, int64_t max_bytes, int64_t* shape_out,
                        int32_t* ndim_out, int32_t* dtype_out) {
    if (!m || !name) {
        cn_set_error("cn_fetch: bad argument");
        return -1;
    }
    const std::string n(name);
    const void* src = nullptr;
    int dtype = CN_DTYPE_F32;
    std::vector<int64_t> shape;
    bool model_prec = false;
    const int64_t B = m->B, Tp = m->Tp, U = m->U, d = m->cfg.d_model;
    auto it = m->captures.find(n);
    const bool stale = it != m->captures.end() && it->second.call != m->call_id;  // captured by an earlier call: not served
    if (it != m->captures.end() && !stale) {
        src = it->second.p;
        dtype = it->second.dtype;
        shape = it->second.shape;
    } else if (n == "best_paths") { src = m->best; dtype = CN_DTYPE_I32; shape = {B, Tp};
    } else if (n == "ctc_maxlp") {
        if (!m->ctc_maxlp_valid) {
            cn_set_error("cn_fetch: ctc_maxlp is only produced by capture runs (the fused CTC generator computes the arg-max alone)");
            return -1;
        }
        src = m->ctc_maxlp; shape = {B, Tp};
    } else if (n == "aligned_seq_shift") { src = m->shift; dtype = CN_DTYPE_I32; shape = {B, Tp};
    } else if (n == "keymask") { src = m->keymask; dtype = CN_DTYPE_U8; shape = {B, Tp};
    } else if (n == "src_size") { src = m->src_size; dtype = CN_DTYPE_I32; shape = {B};
    } else if (n == "ylen") { src = m->ylen; dtype = CN_DTYPE_I32; shape = {B};
    } else if (n == "ymax") { src = m->ymax; dtype = CN_DTYPE_I32; shape = {1};
    } else if (n == "intervals") { src = m->intervals; dtype = CN_DTYPE_I32; shape = {B, Tp + 1, 4};
    } else if ((n == "tok" || n == "val") && m->rows_packed) {
        cn_set_error("cn_fetch: the last pass packed its decoder rows (tok / val are not [B][U]); decode with cn_decode_opts.reserved[1]");
        return -1;
    } else if (n == "tok") { src = m->tok; dtype = CN_DTYPE_I32; shape = {B, U};
    } else if (n == "val") { src = m->val; shape = {B, U};
    } else if (n == "topk_idx") { src = m->topk_idx; dtype = CN_DTYPE_I32; shape = {B, U, m->last_k};
    } else if (n == "topk_val") { src = m->topk_val; shape = {B, U, m->last_k};
    } else if (n == "enc_h_live") { src = m->enc_h; model_prec = true; shape = {B, Tp, d};
    } else if (stale) {
        cn_set_error("cn_fetch: '" + n + "' was captured by an earlier call, not by the last one (capture is a per-call option)");
        return -1;
    } else {
        cn_set_error("cn_fetch: unknown tensor '" + n + "' (captures need opts.capture=1)");
        return -1;
    }
    size_t cnt = 1;
    for (auto v : shape) cnt *= (size_t)v;
    const size_t esz = dtype == CN_DTYPE_U8 ? 1 : (dtype == CN_DTYPE_F64 ? 8 : 4);
    if (shape_out) {
        for (size_t i = 0; i < shape.size() && i < 4; ++i) shape_out[i] = shape[i];
    }
    if (ndim_out) *ndim_out = (int)shape.size();
    if (dtype_out) *dtype_out = dtype;
    if (!host_dst) return 0;  // shape query
    if ((int64_t)(cnt * esz) > max_bytes) {
        cn_set_error("cn_fetch: destination too small");
        return -1;
    }
    CN_HIP_CHECK(hipDeviceSynchronize());
    if (model_prec && m->prec != CN_PREC_F32) {
        float* tmp = nullptr;
        CN_HIP_CHECK(hipMalloc((void**)&tmp, cnt * 4));
        int rc = launch_convert_back(m->prec, src, tmp, cnt, 0);
        if (rc == 0 && hipMemcpy(host_dst, tmp, cnt * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = -2;
        (void)hipFree(tmp);
        if (rc) {
            cn_set_error("cn_fetch: convert/copy failed");
            return rc;
        }
        return 0;
    }
    CN_HIP_CHECK(hipMemcpy(host_dst, src, cnt * esz, hipMemcpyDeviceToHost));
    return 0;
}
