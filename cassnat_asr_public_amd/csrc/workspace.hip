// The device workspace of a handle: one table of its buffers (sizes, allocation, the per-call capacity check), the capture
// copies behind cn_fetch and the named scratch buffers that grow on demand.
#include <algorithm>

#include "model.h"

namespace cn_host {
namespace {

int dev_alloc(cn_model* m, void** p, size_t bytes) {
    if (bytes == 0) bytes = 256;
    CN_HIP_CHECK(hipMalloc(p, bytes));
    m->allocs.push_back(*p);
    return 0;
}

// The workspace table.  One row per buffer: its name (the name of its pointer in cn_model), the bytes it needs for a call of B
// utterances (Bu: for the buffers with one entry per utterance) whose conv1 image has T1 rows and whose encoder has Tp frames,
// with G alignments per utterance on the decoder side, and the assignment of its pointer.  The ONE place these buffers are
// written: build_workspace allocates and assigns them for the configured maxima, in this order, ws_check holds every call
// against what was allocated (round 2's GPU fault was a generator that wrote B x G x U rows into a buffer sized for
// B x (T' + 1): a capacity that only existed implicitly).
struct WsDims {
    size_t B, Bu, T1, Tp, G;
};
struct WsRow {
    const char* name;
    size_t bytes;
    void (*assign)(cn_model*, void*);
};
#define WS_ROW(field, nbytes)                                                                                             \
    do {                                                                                                                  \
        out.push_back({#field, (nbytes), [](cn_model* h, void* p) { h->field = static_cast<decltype(h->field)>(p); }}); \
    } while (0)
std::vector<WsRow> ws_table(const cn_model* m, const WsDims& v) {
    const cn_config& c = m->cfg;
    const size_t es = m->es;
    const size_t B = v.B, T1 = v.T1, Tp = v.Tp, F1 = m->F1, F2 = m->F2, d = c.d_model, V = c.vocab_size, G = v.G;
    const size_t M0 = B * (Tp + 1);  // decoder rows can reach B*(T'+1) per alignment
    const size_t M = M0 * G;
    const size_t dff = std::max(std::max(c.d_encff, c.d_decff), c.d_ff);  // (d_ff: the conformer extractor's FFN width)
    std::vector<WsRow> out;
    WS_ROW(keymask, B * Tp);
    if (c.ast != 2) {  // (the LM has no convolutional front-end)
        WS_ROW(c1, B * (T1 + 2) * (F1 + 2) * d * es);  // room for the zero halo the bf16 conv2 kernel wants
        WS_ROW(c2, B * Tp * F2 * d * es);
    }
    WS_ROW(x, (M + 32) * d * 4);  // + one 32-row block: the chain kernel's blocked layout rounds up
    WS_ROW(xn, (M + 32) * d * es);  // (+ 32 rows: whole 32-row blocks of the chain kernel's blocked LNn(x))
    WS_ROW(qkv, (M + 32) * 3 * d * es);  // (+ 32 rows: the chain kernel writes whole 32-row blocks of its blocked output)
    WS_ROW(ctx, (M + 32) * d * es);  // (+ 32 rows: whole 32-row blocks of the blocked form)
    WS_ROW(hbuf, M * dff * es);
    WS_ROW(enc_h, M0 * d * es);
    WS_ROW(kvm, M0 * 2 * d * es);
    if (m->kv_cols > 0) WS_ROW(kv_all, (M0 + 32) * (size_t)m->kv_cols * es);
    WS_ROW(qd, (M + 32) * d * es);
    WS_ROW(dec_h, M * d * es);
    WS_ROW(xd, (M + 32) * d * 4);
    WS_ROW(xd2, (M + 32) * d * 4);
    WS_ROW(logits, M0 * V * 4);
    WS_ROW(best, M * 4);
    WS_ROW(ctc_maxlp, M0 * 4);
    WS_ROW(shift, M * 4);
    WS_ROW(src_size, v.Bu * G * 4);
    WS_ROW(ylen, v.Bu * G * 4);
    WS_ROW(utt_meta, v.Bu * sizeof(UttMeta));
    WS_ROW(row_off, (v.Bu * G + 1) * 4);
    WS_ROW(ymax, 256);
    WS_ROW(intervals, B * G * (Tp + 1) * 16);
    WS_ROW(tok, M * 4);
    WS_ROW(val, M * 4);
    WS_ROW(topk_idx, M0 * 16 * 4);
    WS_ROW(topk_val, M0 * 16 * 4);
    if (c.conf_enc || c.conf_dec) {  // convolution module: pointwise-conv output [M][2d], depthwise output fp32, GroupNorm sums
        WS_ROW(cv_a, M * 2 * d * es);
        WS_ROW(cv_f, M * d * 4);
        WS_ROW(gn_stats, v.Bu * G * 2 * 8);
    }
    return out;
}
#undef WS_ROW

}  // namespace

int build_workspace(cn_model* m) {
    if (m->keymask) return 0;
    const WsDims dims = {(size_t)m->maxB, (size_t)m->maxU, (size_t)m->maxT1, (size_t)m->maxTp, (size_t)std::max(1, m->cfg.esa_group)};
    for (const WsRow& row : ws_table(m, dims)) {
        void* p = nullptr;
        CN_TRY(dev_alloc(m, &p, row.bytes));
        row.assign(m, p);
        m->ws_cap[row.name] = row.bytes;
    }
    CN_HIP_CHECK(hipHostMalloc((void**)&m->ymax_pinned, 64, hipHostMallocDefault));
    CN_HIP_CHECK(hipHostMalloc((void**)&m->ymax_ring, 64, hipHostMallocDefault));
    bool range_guard = false;
#ifdef CN_OP16_F16
    range_guard = true;
#else
    range_guard = conv2_mix_applies(m->prec, m->cfg.d_model, m->cfg.d_model) && m->cfg.ast != 2;
#endif
    if (range_guard) {
        CN_HIP_CHECK(hipHostMalloc((void**)&m->op16_fault, 64, hipHostMallocMapped));
        *m->op16_fault = 0;
    }
    return 0;
}

// Every buffer of the workspace against what a call of (B utterances, T frames, G alignments per utterance) needs: an error,
// never a write past a buffer.  The workspace is an AREA (max_batch x max_frames): more, shorter utterances fit as well.
int ws_check(cn_model* m, int B, int T, int G, const char* what) {
    const int T1 = (T - 1) / 2 + 1, Tp = (T1 - 1) / 2 + 1;
    for (const WsRow& row : ws_table(m, {(size_t)B, (size_t)B, (size_t)T1, (size_t)Tp, (size_t)std::max(1, G)})) {
        auto it = m->ws_cap.find(row.name);
        if (it == m->ws_cap.end() || row.bytes > it->second) {
            cn_set_error(std::string(what) + ": workspace buffer '" + row.name + "' holds " +
                         std::to_string(it == m->ws_cap.end() ? 0 : it->second) + " bytes, the call (B=" + std::to_string(B) + " T=" +
                         std::to_string(T) + " alignments=" + std::to_string(G) + ") needs " + std::to_string(row.bytes) +
                         " (workspace: max_batch " + std::to_string(m->maxB) + " x max_frames " + std::to_string(m->maxT) + ")");
            return -1;
        }
    }
    if (Tp + 1 > m->pe_rows) {
        cn_set_error(std::string(what) + ": more subsampled frames than the positional table has rows");
        return -1;
    }
    return 0;
}

int capture(cn_model* m, const char* name, const void* src, bool model_prec, int dtype, std::vector<int64_t> shape,
            hipStream_t s) {
    size_t n = 1;
    for (auto v : shape) n *= (size_t)v;
    const size_t esz = dtype == CN_DTYPE_U8 ? 1 : (dtype == CN_DTYPE_F64 ? 8 : 4);
    Capture& cp = m->captures[name];
    if (cp.bytes < n * esz) {
        if (cp.p) (void)hipFree(cp.p);
        CN_HIP_CHECK(hipMalloc(&cp.p, n * esz));
        cp.bytes = n * esz;
    }
    cp.dtype = dtype;
    cp.shape = shape;
    cp.call = m->call_id;
    if (model_prec)
        CN_TRY(launch_convert_back(m->prec, src, (float*)cp.p, n, s));
    else
        CN_HIP_CHECK(hipMemcpyAsync(cp.p, src, n * esz, hipMemcpyDeviceToDevice, s));
    return 0;
}

int scratch_buf(cn_model* m, const char* name, size_t bytes, void** out) {
    auto& e = m->scratch[name];
    if (e.second < bytes) {
        if (e.first) (void)hipFree(e.first);
        e.first = nullptr;
        e.second = 0;
        CN_HIP_CHECK(hipMalloc(&e.first, bytes));
        e.second = bytes;
    }
    *out = e.first;
    return 0;
}

}  // namespace cn_host
