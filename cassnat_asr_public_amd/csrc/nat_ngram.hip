// CASS-NAT finish loop with word n-gram shallow fusion for gfx950: `--task cassnat`, `lm_weight > 0`, `rank_model: n-gram`, an ARPA
// model.  The reference fuses only a TransformerLM there (natlm.hip); this is the class-term fusion of ast_ngram_search.h in
// CassNAT.beam_decode's finish loop.  nat_ngram_search.h holds the step functions, include/cassnat_hip_nat_ngram.h the contract.
//
// Two launches for a whole batch.  nat_class_topk_kernel ranks every row of the pass once, per class, independent of the beam: it is
// the only code that reads the B * U * V floats.  nat_ngram_finish_kernel then runs all steps of one utterance in one workgroup on
// O(beam) state in LDS - per slot an AnState, a double score and the newest token, double buffered by parity - and the class tables;
// the token history goes to a global scratch of (token, parent slot) pairs, which the same workgroup back-traces at the end.
// Every loop is bounded: the step loop by last[b] (clamped on entry), the probe loops by their tables' slot counts; every barrier is
// reached by the whole workgroup (last[b] is uniform over it).
#include "kernels.h"
#include "model.h"
#include "nat_ngram_search.h"
#include "rowreduce.h"

using namespace cn_host;

// One workgroup per row (b, i), i <= last[b].  The row is staged in LDS once per class with the entries of the other classes as NaNs,
// which rr_select_rounds never chooses; k rounds select by (value descending, index ascending).  A thread stages and rescans only the
// entries it owns (c = tid mod 256), so no barrier stands between the staging and the rounds.
__global__ __launch_bounds__(256) void nat_class_topk_kernel(const float* __restrict__ att, const int* __restrict__ last,
                                                             const int* __restrict__ zlen, int U, int V,
                                                             const unsigned char* __restrict__ starts, int eos, int k,
                                                             int* __restrict__ cls_idx, float* __restrict__ cls_val,
                                                             float* __restrict__ eos_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ RowReduceLds red;
    const int r = blockIdx.x, b = r / U, i = r - b * U, tid = threadIdx.x;
    const int l = last[b] < U - 1 ? last[b] : U - 1;
    if (i > l) return;  // (the whole workgroup leaves, before any barrier)
    const bool zero = zlen && i >= zlen[b];
    const float* pa = att + (long long)r * V;
    const float nan = __builtin_nanf("");
    for (int cls = 0; cls < 2; ++cls) {
        for (int c = tid; c < V; c += 256) row[c] = nn_class(starts, eos, c) == cls ? (zero ? 0.f : pa[c]) : nan;
        int* oi = cls_idx + ((long long)r * 2 + cls) * k;
        float* ov = cls_val + ((long long)r * 2 + cls) * k;
        rr_select_rounds(red, row, V, tid, k, nan, [&](int round, int bidx, float best) {
            oi[round] = bidx < V ? bidx : -1;  // (a class with fewer than k members)
            ov[round] = bidx < V ? best : -INFINITY;
        });
    }
    if (tid == 0) eos_val[r] = zero ? 0.f : pa[eos];
}

struct NnFinishArgs {
    cn_ngram_desc d;
    float scale;
    const int* cls_idx;    // [B][U][2][bw]
    const float* cls_val;  // [B][U][2][bw]
    const float* eos_val;  // [B][U]
    const int* last;       // [B]
    int U, bw, eos, sos, pad, use_lp, L;
    double lp;
    int* hist;      // [B][U][bw][2] (token, parent slot)
    int* hyp;       // [B][bw][L]
    int* hyp_len;   // [B][bw]
    double* score;  // [B][bw]
};

// One workgroup per utterance, all of its steps.  Per step: every live slot advances its state by its newest token; lanes do the
// 2 * NG_TASKS probes of every slot; one lane per slot sums them and merges the slot's candidates; one thread per candidate forms its
// key and its rank (nat_beam_update_kernel's); one thread per new slot copies its parent's state to the other parity.
__global__ __launch_bounds__(NN_MAXC) void nat_ngram_finish_kernel(NnFinishArgs a) {
    __shared__ AnState st[2][NN_MAXW];
    __shared__ double sc[2][NN_MAXW];
    __shared__ int newest[2][NN_MAXW];
    __shared__ NgProbe pr[NN_MAXW][2 * NG_TASKS];
    __shared__ float adds[NN_MAXW][2];
    __shared__ double ckey[NN_MAXC], cscore[NN_MAXC];
    __shared__ int ctok[NN_MAXC], newslot[NN_MAXW];
    __shared__ float cval[NN_MAXC];
    const int b = blockIdx.x, tid = threadIdx.x, bw = a.bw, U = a.U;
    const int last = nn_clamp_last(a.last[b], U, a.L);
    if (tid == 0) an_init(a.d, &st[0][0]);
    if (tid < NN_MAXW) sc[0][tid] = 0.0, newest[0][tid] = 0;
    __syncthreads();
    int cur = 0;
    for (int step = 0; step <= last; ++step) {
        const int nl = step == 0 ? 1 : bw, ncand = nl * bw, nxt = cur ^ 1;
        const long long r = (long long)b * U + step;
        if (tid < nl) nn_advance(a.d, &st[cur][tid], step > 0, newest[cur][tid], a.eos);
        if (tid < NN_MAXW) newslot[tid] = 0;  // (NaN keys rank nowhere: every slot still names a candidate of this utterance)
        __syncthreads();
        for (int t = tid; t < nl * 2 * NG_TASKS; t += NN_MAXC) an_probe(a.d, st[cur][t / (2 * NG_TASKS)], t % (2 * NG_TASKS), &pr[t / (2 * NG_TASKS)][t % (2 * NG_TASKS)]);
        __syncthreads();
        if (tid < nl) {
            an_adds(a.d, st[cur][tid], pr[tid], adds[tid]);
            nn_merge(a.cls_idx + r * 2 * bw, a.cls_val + r * 2 * bw, a.eos_val[r], a.eos, adds[tid], a.scale, bw, &ctok[tid * bw], &cval[tid * bw]);
        }
        __syncthreads();
        if (tid < ncand) {
            const double s = sc[cur][tid / bw] + (double)cval[tid];
            cscore[tid] = s;
            ckey[tid] = nn_key(s, step, a.use_lp, a.lp);
        }
        __syncthreads();
        if (tid < ncand) {
            const int rank = nn_rank(ckey, ncand, tid);
            if (rank < bw) newslot[rank] = tid;
        }
        __syncthreads();
        if (tid < bw) {
            const int e = newslot[tid], parent = e / bw;
            st[nxt][tid] = st[cur][parent];
            sc[nxt][tid] = cscore[e];
            newest[nxt][tid] = ctok[e];
            a.hist[(r * bw + tid) * 2] = ctok[e];
            a.hist[(r * bw + tid) * 2 + 1] = parent;
        }
        __syncthreads();
        cur = nxt;
    }
    if (tid < bw) {
        int* h = a.hyp + ((long long)b * bw + tid) * a.L;
        h[0] = a.sos;
        for (int t = last + 2; t < a.L; ++t) h[t] = a.pad;
        int slot = tid;
        for (int i = last; i >= 0; --i) {
            const long long o = (((long long)b * U + i) * bw + slot) * 2;
            h[i + 1] = a.hist[o];
            const int p = a.hist[o + 1];
            slot = p < 0 ? 0 : (p >= bw ? bw - 1 : p);  // (the scratch is this workgroup's own writing; the clamp keeps the walk inside it)
        }
        a.hyp_len[b * bw + tid] = last + 2;
        a.score[b * bw + tid] = sc[cur][tid];
    }
}

// last[b] = min(ylen[b], ymax - 1): the last step utterance b consumes (natlm.hip: nat_beam_init_kernel)
__global__ void nat_ngram_last_kernel(const int* __restrict__ ylen, int ymax, int B, int* __restrict__ last) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) last[b] = ylen[b] < ymax - 1 ? ylen[b] : ymax - 1;
}

static int launch_nat_class_topk(const float* att, const int* last, const int* zlen, int B, int U, int V, const unsigned char* starts, int eos,
                                 int k, int* cls_idx, float* cls_val, float* eos_val, hipStream_t s) {
    const std::string bad = nn_check(B, U, V, k, eos, 1);
    if (!bad.empty()) {
        cn_set_error("nat_class_topk: " + bad);
        return -1;
    }
    if ((long long)B * U > 0x7fffffffll) {
        cn_set_error("nat_class_topk: too many rows");
        return -1;
    }
    hipLaunchKernelGGL(nat_class_topk_kernel, dim3((unsigned)(B * U)), dim3(256), (size_t)V * sizeof(float), s, att, last, zlen, U, V, starts,
                       eos, k, cls_idx, cls_val, eos_val);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

static int launch_nat_ngram_finish(const NnFinishArgs& a, int B, int V, hipStream_t s) {
    std::string bad = ng_check_desc(a.d);
    if (bad.empty()) bad = nn_check(B, a.U, V, a.bw, a.eos, a.L);
    if (bad.empty() && (!(a.scale == a.scale) || !(a.lp == a.lp))) bad = "lm_scale and length_penalty must be numbers";
    if (!bad.empty()) {
        cn_set_error("nat_ngram_finish: " + bad);
        return -1;
    }
    hipLaunchKernelGGL(nat_ngram_finish_kernel, dim3((unsigned)B), dim3(NN_MAXC), 0, s, a);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int cn_nat_attach_ngram(cn_model* m, const cn_ngram_desc* desc, float lm_scale) {
    if (!m || m->cfg.ast != 0) {
        cn_set_error("cn_nat_attach_ngram: the handle must be a CASS-NAT model (cfg.ast = 0)");
        return -1;
    }
    if (!desc) {
        m->ast_ng_on = false;
        m->ast_ng = cn_ngram_desc{};
        m->ast_ng_scale = 0.f;
        return 0;
    }
    if (m->ast_lm) {
        cn_set_error("cn_nat_attach_ngram: a TransformerLM is attached (cn_nat_attach_lm); it and an n-gram model cannot be fused together");
        return -1;
    }
    const std::string bad = ng_check_desc(*desc);
    if (!bad.empty()) {
        cn_set_error("cn_nat_attach_ngram: " + bad);
        return -1;
    }
    if (desc->vocab != m->cfg.vocab_size) {
        cn_set_error("cn_nat_attach_ngram: the model's pieces must be the decoder's vocabulary (desc->vocab " + std::to_string(desc->vocab) +
                     ", vocab_size " + std::to_string(m->cfg.vocab_size) + ")");
        return -1;
    }
    if (!(lm_scale == lm_scale)) {
        cn_set_error("cn_nat_attach_ngram: lm_scale must be a number");
        return -1;
    }
    m->ast_ng = *desc;
    m->ast_ng_scale = lm_scale;
    m->ast_ng_on = true;
    return 0;
}

extern "C" int cn_nat_ngram_finish(cn_model* m, const cn_decode_opts* opts, int32_t ymax, int32_t beam_width, int32_t eos,
                                   int32_t use_length_penalty, double length_penalty, int32_t zero_past_len, int32_t* hyp_out_dev,
                                   int32_t max_len, int32_t* hyp_len_dev, double* score_dev, void* stream) {
    if (!m || !opts || !hyp_out_dev || !hyp_len_dev || !score_dev) {
        cn_set_error("cn_nat_ngram_finish: null argument");
        return -1;
    }
    if (m->cfg.ast != 0 || !m->ast_ng_on) {
        cn_set_error("cn_nat_ngram_finish: needs an n-gram model attached with cn_nat_attach_ngram");
        return -1;
    }
    const int bw = beam_width, B = m->B, U = m->att_rows_U, V = m->cfg.vocab_size, L = max_len;
    if (U < 1 || B < 1) {
        cn_set_error("cn_nat_ngram_finish: the last decode pass kept no log-probability rows (set cn_decode_opts.reserved[0], one "
                     "alignment per utterance)");
        return -1;
    }
    if (bw < 1 || bw > NN_MAXW || bw > V || ymax < 1 || ymax > U || L < ymax + 1) {
        cn_set_error("cn_nat_ngram_finish: need 1 <= beam_width <= 16, 1 <= ymax <= rows of the pass and max_len >= ymax + 1");
        return -1;
    }
    const std::string bad = nn_check(B, U, V, bw, eos, L);
    if (!bad.empty()) {
        cn_set_error("cn_nat_ngram_finish: " + bad);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    const size_t rows = (size_t)B * U;
    int *last = nullptr, *cidx = nullptr, *hist = nullptr;
    float *cval = nullptr, *ev = nullptr;
    CN_TRY(scratch_buf(m, "nng_last", (size_t)B * 4, (void**)&last));
    CN_TRY(scratch_buf(m, "nng_cls_idx", rows * 2 * bw * 4, (void**)&cidx));
    CN_TRY(scratch_buf(m, "nng_cls_val", rows * 2 * bw * 4, (void**)&cval));
    CN_TRY(scratch_buf(m, "nng_eos_val", rows * 4, (void**)&ev));
    CN_TRY(scratch_buf(m, "nng_hist", rows * bw * 2 * 4, (void**)&hist));
    hipLaunchKernelGGL(nat_ngram_last_kernel, dim3(cn_ceil_div(B, 64)), dim3(64), 0, s, m->ylen, ymax, B, last);
    CN_HIP_CHECK(hipGetLastError());
    {
        ProfScope ps(m, "nat_class_topk", 0, (double)rows * V * 4, s);
        CN_TRY(launch_nat_class_topk(m->logits, last, zero_past_len ? m->ylen : nullptr, B, U, V, m->ast_ng.piece_starts, eos, bw, cidx, cval, ev, s));
    }
    NnFinishArgs a;
    a.d = m->ast_ng;
    a.scale = m->ast_ng_scale;
    a.cls_idx = cidx, a.cls_val = cval, a.eos_val = ev, a.last = last;
    a.U = U, a.bw = bw, a.eos = eos, a.sos = opts->sos, a.pad = opts->padding_idx, a.use_lp = use_length_penalty, a.L = L;
    a.lp = length_penalty;
    a.hist = hist, a.hyp = hyp_out_dev, a.hyp_len = hyp_len_dev, a.score = score_dev;
    ProfScope ps(m, "nat_ngram_finish", 0, (double)rows * (4 * bw + 1) * 4, s);
    return launch_nat_ngram_finish(a, B, V, s);
}

extern "C" int cn_op_nat_class_topk(const float* att, const int32_t* last, const int32_t* zlen, int32_t B, int32_t U, int32_t V,
                                    const uint8_t* starts, int32_t eos, int32_t k, int32_t* cls_idx, float* cls_val, float* eos_val,
                                    void* stream) {
    if (!att || !last || !starts || !cls_idx || !cls_val || !eos_val) {
        cn_set_error("cn_op_nat_class_topk: null argument");
        return -1;
    }
    return launch_nat_class_topk(att, last, zlen, B, U, V, starts, eos, k, cls_idx, cls_val, eos_val, (hipStream_t)stream);
}

extern "C" int cn_op_nat_ngram_finish(const cn_ngram_desc* desc, float lm_scale, const int32_t* cls_idx, const float* cls_val,
                                      const float* eos_val, const int32_t* last, int32_t B, int32_t U, int32_t beam_width, int32_t eos,
                                      int32_t sos, int32_t pad, int32_t use_length_penalty, double length_penalty, int32_t* hist, int32_t* hyp,
                                      int32_t max_len, int32_t* hyp_len, double* score, void* stream) {
    if (!desc || !cls_idx || !cls_val || !eos_val || !last || !hist || !hyp || !hyp_len || !score) {
        cn_set_error("cn_op_nat_ngram_finish: null argument");
        return -1;
    }
    NnFinishArgs a;
    a.d = *desc;
    a.scale = lm_scale;
    a.cls_idx = cls_idx, a.cls_val = cls_val, a.eos_val = eos_val, a.last = last;
    a.U = U, a.bw = beam_width, a.eos = eos, a.sos = sos, a.pad = pad, a.use_lp = use_length_penalty, a.L = max_len;
    a.lp = length_penalty;
    a.hist = hist, a.hyp = hyp, a.hyp_len = hyp_len, a.score = score;
    return launch_nat_ngram_finish(a, B, desc->vocab, (hipStream_t)stream);  // (the tables cover desc->vocab pieces)
}

// the same step functions on the host: every pointer a host pointer, no GPU call
extern "C" int cn_nat_ngram_finish_host(const cn_ngram_desc* desc, float lm_scale, const float* att, const int32_t* ylen, const int32_t* zlen,
                                        int32_t B, int32_t U, int32_t V, int32_t ymax, int32_t beam_width, int32_t eos, int32_t sos,
                                        int32_t pad, int32_t use_length_penalty, double length_penalty, int32_t* hyp, int32_t max_len,
                                        int32_t* hyp_len, double* score) {
    if (!desc || !att || !ylen || !hyp || !hyp_len || !score) {
        cn_set_error("cn_nat_ngram_finish_host: null argument");
        return -1;
    }
    std::string bad = ng_check_desc(*desc);
    if (bad.empty()) bad = nn_check(B, U, V, beam_width, eos, max_len);
    if (bad.empty() && desc->vocab != V) bad = "the model's pieces must be the rows' vocabulary";
    if (bad.empty() && (ymax < 1 || ymax > U || max_len < ymax + 1)) bad = "need 1 <= ymax <= U and max_len >= ymax + 1";
    if (bad.empty() && (!(lm_scale == lm_scale) || !(length_penalty == length_penalty))) bad = "lm_scale and length_penalty must be numbers";
    if (!bad.empty()) {
        cn_set_error("cn_nat_ngram_finish_host: " + bad);
        return -1;
    }
    NnHostArgs a;
    a.d = *desc, a.scale = lm_scale, a.att = att, a.ylen = ylen, a.zlen = zlen;
    a.B = B, a.U = U, a.V = V, a.ymax = ymax, a.bw = beam_width, a.eos = eos, a.sos = sos, a.pad = pad, a.use_lp = use_length_penalty, a.L = max_len;
    a.lp = length_penalty;
    a.hyp = hyp, a.hyp_len = hyp_len, a.score = score;
    for (int b = 0; b < B; ++b) nn_search_host(a, b);
    return 0;
}
