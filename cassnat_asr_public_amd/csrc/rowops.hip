// Row-wise, HBM-bound kernels of the hot path: the reference's custom LayerNorm, the generator's
// log-softmax + argmax, the padding mask, query-table broadcast and precision converts.
#include "feats_compress.h"
#include "kernels.h"
#include "rowreduce.h"

// ---------------------------------------------------------------------------------------------
// LayerNorm exactly as src/models/modules/norm.py:15-18: unbiased std (divide by d-1), eps added to
// the std (not the variance).  One wave per row, 16 bytes per lane per step, two-pass in registers.
// ---------------------------------------------------------------------------------------------
template <typename TY>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ a2,
                                                        const float* __restrict__ b2, TY* __restrict__ y, int M, int d,
                                                        float eps, float out_scale) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (long long)row * d;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = (i * 64 + lane) * 4;
        if (idx < d) {
            v[i] = *reinterpret_cast<const f32x4*>(xr + idx);
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean = wave_sum(s) / (float)d;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = (i * 64 + lane) * 4;
        if (idx < d) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float c = v[i][j] - mean;
                ss = fmaf(c, c, ss);
            }
        }
    }
    const float denom = sqrtf(wave_sum(ss) / (float)(d - 1)) + eps;
    TY* yr = y + (long long)row * d;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = (i * 64 + lane) * 4;
        if (idx < d) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(a2 + idx);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(b2 + idx);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = g[j] * (v[i][j] - mean) / denom + bb[j];
            if constexpr (sizeof(TY) == 1) {  // e4m3fn at the consumer's per-tensor scale (config 5)
                unsigned int w = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) w |= (unsigned int)cn_f32_to_fp8(o[j] * out_scale) << (8 * j);
                *reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(yr) + idx) = w;
            } else if constexpr (sizeof(TY) == 2) {
                bf16x4 ob;
#pragma unroll
                for (int j = 0; j < 4; ++j) ob[j] = (bf16)o[j];
                *reinterpret_cast<bf16x4*>(yr + idx) = ob;
            } else if constexpr (__is_same(TY, split_t)) {  // hi / lo halves of the element's 32-group (common.h)
                bf16x4 hi, lo;
                cn_split4(o, hi, lo);
                unsigned char* yb = reinterpret_cast<unsigned char*>(yr) + cn_split_off((size_t)idx);
                *reinterpret_cast<bf16x4*>(yb) = hi;
                *reinterpret_cast<bf16x4*>(yb + 64) = lo;
            } else {
                f32x4 of;
#pragma unroll
                for (int j = 0; j < 4; ++j) of[j] = o[j];
                *reinterpret_cast<f32x4*>(yr + idx) = of;
            }
        }
    }
}

int launch_layernorm(int prec, const float* x, const float* a2, const float* b2, void* y, int y_f32, int M, int d,
                     float eps, hipStream_t s) {
    if (d % 4 != 0 || d > 1024 || d < 2) {
        cn_set_error("layernorm: d must be a multiple of 4 in [4, 1024]");
        return -1;
    }
    if (M <= 0) return 0;
    const dim3 grid(cn_ceil_div(M, 4));
    if (prec == CN_PREC_X3 && !y_f32 && d % 32 != 0) {
        cn_set_error("layernorm: split-bf16 rows need d % 32 == 0");
        return -1;
    }
    if (y_f32 || prec == CN_PREC_F32)
        hipLaunchKernelGGL(layernorm_kernel<float>, grid, dim3(256), 0, s, x, a2, b2, (float*)y, M, d, eps, 1.f);
    else if (prec == CN_PREC_X3)
        hipLaunchKernelGGL(layernorm_kernel<split_t>, grid, dim3(256), 0, s, x, a2, b2, (split_t*)y, M, d, eps, 1.f);
    else
        hipLaunchKernelGGL(layernorm_kernel<bf16>, grid, dim3(256), 0, s, x, a2, b2, (bf16*)y, M, d, eps, 1.f);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// LayerNorm straight into e4m3fn at `scale` (the A operand of an fp8 product)
int launch_layernorm_fp8(const float* x, const float* a2, const float* b2, void* y, int M, int d, float eps, float scale,
                         hipStream_t s) {
    if (d % 4 != 0 || d > 1024 || d < 2) {
        cn_set_error("layernorm: d must be a multiple of 4 in [4, 1024]");
        return -1;
    }
    if (M <= 0) return 0;
    hipLaunchKernelGGL(layernorm_kernel<fp8_t>, dim3(cn_ceil_div(M, 4)), dim3(256), 0, s, x, a2, b2, (fp8_t*)y, M, d, eps, scale);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// bf16 [M][K] (row stride ld) -> e4m3fn [M][K] at `scale`, saturating: the A operand of an fp8 product whose producer
// writes bf16 (the attention context)
__global__ void quantize_fp8_kernel(const bf16* __restrict__ src, int ld, unsigned char* __restrict__ dst, int M, int K, float scale) {
    const long long n4 = (long long)M * (K / 4);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / (K / 4);
        const int c = (int)(i - m * (K / 4)) * 4;
        const bf16x4 v = *reinterpret_cast<const bf16x4*>(src + m * ld + c);
        unsigned int w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= (unsigned int)cn_f32_to_fp8((float)v[j] * scale) << (8 * j);
        *reinterpret_cast<unsigned int*>(dst + m * K + c) = w;
    }
}
int launch_quantize_fp8(const void* src_bf16, int ld, void* dst, int M, int K, float scale, hipStream_t s) {
    if (M <= 0 || K <= 0) return 0;
    if (K % 4 != 0 || ld % 4 != 0) {
        cn_set_error("quantize_fp8: K and the row stride must be multiples of 4");
        return -1;
    }
    const long long n4 = (long long)M * (K / 4);
    long long g = (n4 + 255) / 256;
    if (g > 65536) g = 65536;
    hipLaunchKernelGGL(quantize_fp8_kernel, dim3((unsigned)g), dim3(256), 0, s, (const bf16*)src_bf16, ld, (unsigned char*)dst, M, K, scale);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Generator tail (src/models/cassnat.py:113 log_softmax, :378 argmax, :611 topk(1)): per row of
// fp32 logits the first-index argmax and its log-probability (x - max) - log(sum exp(x - max));
// optionally the row is rewritten in place as log-probabilities.  One workgroup per row.  The
// reductions of this and the three kernels below are rowreduce.h's: one partition, one order.
// ---------------------------------------------------------------------------------------------
// temperature: Generator.forward(x, T) = log_softmax(proj(x) / T) (src/models/transformer.py:48-51); 1.0 = no division
__global__ __launch_bounds__(256) void logsoftmax_argmax_kernel(float* __restrict__ logits, int V, int ldl,
                                                                int* __restrict__ arg, float* __restrict__ maxlp,
                                                                int write_logp, float temperature) {
    __shared__ RowReduceLds red;
    float* p = logits + (long long)blockIdx.x * ldl;
    const int tid = threadIdx.x;
    if (temperature != 1.0f) {
        for (int i = tid; i < V; i += 256) p[i] = p[i] / temperature;
        __syncthreads();
    }
    float best;
    int bidx;
    rr_local_best(p, V, tid, best, bidx);
    rr_block_argmax(red, tid, best, bidx);
    const float lse = rr_block_lse(red, p, V, tid, best);
    if (tid == 0) {
        arg[blockIdx.x] = bidx;
        maxlp[blockIdx.x] = -lse;
    }
    if (write_logp)
        for (int i = tid; i < V; i += 256) p[i] = (p[i] - best) - lse;
}

int launch_logsoftmax_argmax(float* logits, int M, int V, int ldl, int* arg, float* maxlp, int write_logp,
                             hipStream_t s) {
    if (M <= 0) return 0;
    hipLaunchKernelGGL(logsoftmax_argmax_kernel, dim3(M), dim3(256), 0, s, logits, V, ldl, arg, maxlp, write_logp, 1.0f);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_logsoftmax_temp(float* logits, int M, int V, int ldl, float temperature, int* arg, float* maxlp, hipStream_t s) {
    if (M <= 0) return 0;
    hipLaunchKernelGGL(logsoftmax_argmax_kernel, dim3(M), dim3(256), 0, s, logits, V, ldl, arg, maxlp, 1, temperature);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// per-row top-k of log-probs (beam_width > 1, src/models/cassnat.py:611). Row staged in LDS (every thread its own entries), k rounds.
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ logp, int V, int ldl, int k,
                                                   int* __restrict__ idx, float* __restrict__ val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ RowReduceLds red;
    const float* p = logp + (long long)blockIdx.x * ldl;
    const int tid = threadIdx.x;
    for (int i = tid; i < V; i += 256) row[i] = p[i];
    rr_select_rounds(red, row, V, tid, k, -INFINITY, [&](int r, int bidx, float best) {
        idx[(long long)blockIdx.x * k + r] = bidx;
        val[(long long)blockIdx.x * k + r] = best;
    });
}

int launch_topk(const float* logp, int M, int V, int ldl, int k, int* idx, float* val, hipStream_t s) {
    if (k < 1 || k > 64 || k > V || V > 16384) {
        cn_set_error("topk: need 1 <= k <= min(64, V) and V <= 16384");
        return -1;
    }
    if (M <= 0) return 0;
    hipLaunchKernelGGL(topk_kernel, dim3(M), dim3(256), (size_t)V * sizeof(float), s, logp, V, ldl, k, idx, val);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// Generator tail of the autoregressive step in one pass per row: log_softmax(logits / T) and its top-k (sorted descending,
// ties: lower index first).  Same per-element arithmetic as logsoftmax_argmax_kernel followed by topk_kernel - x / T, the
// row maximum, the sum of expf(x - max) in the same partition and order, (x - max) - lse per entry (in LDS) - without
// writing the (M, V) log-probabilities back and with the k selection rounds working on cached per-thread maxima (only the
// thread that owned the previous winner rescans its V / 256 entries).
//
// FUSE (LM shallow fusion without CTC, src/models/transformer.py:190-192, 214): a second row `lm` of LM logits (temperature 1)
// is staged beside it; its own maximum and log-sum-exp (same partition and order), then every entry becomes
// att_logp + fl(w * lm_logp) in float32 with one rounding per operation (torch's `att_prob + lm_weight * lm_prob`), and the k
// rounds select on that sum - the candidate set is the fused one, not the attention top-k.
template <bool FUSE>
__global__ __launch_bounds__(256) void logsoftmax_topk_kernel(const float* __restrict__ logits, int V, int ldl, float temperature,
                                                              int k, int* __restrict__ idx, float* __restrict__ val,
                                                              const float* __restrict__ lm, float w) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ RowReduceLds red;
    const float* p = logits + (long long)blockIdx.x * ldl;
    const int tid = threadIdx.x;
    if (temperature != 1.0f)
        for (int i = tid; i < V; i += 256) row[i] = p[i] / temperature;
    else
        for (int i = tid; i < V; i += 256) row[i] = p[i];
    float rmax;
    int rarg;
    rr_local_best(row, V, tid, rmax, rarg);
    rr_block_argmax(red, tid, rmax, rarg);
    const float lse = rr_block_lse(red, row, V, tid, rmax);
    // the selection ranks the LOG-PROBABILITIES, as the two-kernel form and the reference do: two logits one ulp apart can
    // round to the same log-probability, and the tie then goes to the lower index
    if constexpr (FUSE) {
        float* lrow = row + V;
        const float* pl = lm + (long long)blockIdx.x * ldl;
        float lbest = -INFINITY;
        for (int i = tid; i < V; i += 256) {
            const float v = pl[i];
            lrow[i] = v;
            lbest = fmaxf(lbest, v);
        }
        const float lmax = rr_block_max(red, tid, lbest);
        const float llse = rr_block_lse(red, lrow, V, tid, lmax);
        for (int i = tid; i < V; i += 256)
            row[i] = __fadd_rn(__fsub_rn(__fsub_rn(row[i], rmax), lse), cn_mul_rn(w, __fsub_rn(__fsub_rn(lrow[i], lmax), llse)));
    } else {
        for (int i = tid; i < V; i += 256) row[i] = (row[i] - rmax) - lse;
    }
    rr_select_rounds(red, row, V, tid, k, -INFINITY, [&](int r, int bidx, float best) {
        idx[(long long)blockIdx.x * k + r] = bidx;
        val[(long long)blockIdx.x * k + r] = best;
    });
}

int launch_logsoftmax_topk(const float* logits, int M, int V, int ldl, float temperature, int k, int* idx, float* val,
                           hipStream_t s) {
    if (k < 1 || k > 32 || k > V || V > 16384) {  // (k > V: a round would pick a retired entry again)
        cn_set_error("logsoftmax_topk: need 1 <= k <= min(32, V) and V <= 16384");
        return -1;
    }
    if (M <= 0) return 0;
    hipLaunchKernelGGL(logsoftmax_topk_kernel<false>, dim3(M), dim3(256), (size_t)V * sizeof(float), s, logits, V, ldl, temperature, k,
                       idx, val, nullptr, 0.f);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_logsoftmax_fuse_topk(const float* att, const float* lm, int M, int V, int ldl, float temperature, float w, int k,
                                int* idx, float* val, hipStream_t s) {
    if (k < 1 || k > 32 || k > V || V > 8192) {
        cn_set_error("logsoftmax_fuse_topk: need 1 <= k <= min(32, V) and V <= 8192");
        return -1;
    }
    if (M <= 0) return 0;
    hipLaunchKernelGGL(logsoftmax_topk_kernel<true>, dim3(M), dim3(256), (size_t)2 * V * sizeof(float), s, att, V, ldl, temperature, k,
                       idx, val, lm, w);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// Word n-gram shallow fusion without CTC (include/cassnat_hip_ast_ngram.h): logsoftmax_topk_kernel<true>'s sibling.  The second
// addend of entry c is no LM row but fl32(w * term(c)), term(c) one of three numbers: adds[row][1] for eos, adds[row][0] for a piece
// that begins with a separator (starts[c]), 0 for every other.  The row arithmetic before it - x / T, maximum, log-sum-exp,
// (x - max) - lse - and the selection after it are logsoftmax_topk_kernel's, so zero adds give its output bit for bit.
__global__ __launch_bounds__(256) void logsoftmax_class_topk_kernel(const float* __restrict__ logits, int V, int ldl, float temperature,
                                                                    int k, int* __restrict__ idx, float* __restrict__ val,
                                                                    const unsigned char* __restrict__ starts,
                                                                    const float* __restrict__ adds, int eos, float w) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ RowReduceLds red;
    const float* p = logits + (long long)blockIdx.x * ldl;
    const int tid = threadIdx.x;
    if (temperature != 1.0f)
        for (int i = tid; i < V; i += 256) row[i] = p[i] / temperature;
    else
        for (int i = tid; i < V; i += 256) row[i] = p[i];
    float rmax;
    int rarg;
    rr_local_best(row, V, tid, rmax, rarg);
    rr_block_argmax(red, tid, rmax, rarg);
    const float lse = rr_block_lse(red, row, V, tid, rmax);
    const float a_word = cn_mul_rn(w, adds[2 * (long long)blockIdx.x]), a_eos = cn_mul_rn(w, adds[2 * (long long)blockIdx.x + 1]);
    const float a_none = cn_mul_rn(w, 0.f);
    for (int i = tid; i < V; i += 256)
        row[i] = __fadd_rn(__fsub_rn(__fsub_rn(row[i], rmax), lse), i == eos ? a_eos : (starts[i] ? a_word : a_none));
    rr_select_rounds(red, row, V, tid, k, -INFINITY, [&](int r, int bidx, float best) {
        idx[(long long)blockIdx.x * k + r] = bidx;
        val[(long long)blockIdx.x * k + r] = best;
    });
}

int launch_logsoftmax_class_topk(const float* att, int M, int V, int ldl, float temperature, const unsigned char* starts,
                                 const float* adds, int eos, float w, int k, int* idx, float* val, hipStream_t s) {
    if (k < 1 || k > 32 || k > V || V > 8192) {
        cn_set_error("logsoftmax_class_topk: need 1 <= k <= min(32, V) and V <= 8192");
        return -1;
    }
    if (M <= 0) return 0;
    hipLaunchKernelGGL(logsoftmax_class_topk_kernel, dim3(M), dim3(256), (size_t)V * sizeof(float), s, att, V, ldl, temperature, k, idx,
                       val, starts, adds, eos, w);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// LM shallow fusion with CTC (src/models/transformer.py:208-209, lm_prob.gather(1, indices)): per row the log-sum-exp of the LM
// logits (temperature 1; rowreduce.h, as in logsoftmax_topk_kernel), then out[r][c] = (x[cand[r][c]] - max) - lse for
// the k attention candidates.  One workgroup per row; the row is read once, into LDS.
__global__ __launch_bounds__(256) void logsoftmax_gather_kernel(const float* __restrict__ logits, int V, int ldl,
                                                                const int* __restrict__ cand, int k, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ RowReduceLds red;
    const float* p = logits + (long long)blockIdx.x * ldl;
    const int tid = threadIdx.x;
    float best = -INFINITY;
    for (int i = tid; i < V; i += 256) {
        const float v = p[i];
        row[i] = v;
        best = fmaxf(best, v);
    }
    const float rmax = rr_block_max(red, tid, best);
    const float lse = rr_block_lse(red, row, V, tid, rmax);
    if (tid < k) {
        const int c = cand[(long long)blockIdx.x * k + tid];
        out[(long long)blockIdx.x * k + tid] = (c >= 0 && c < V) ? (row[c] - rmax) - lse : -INFINITY;
    }
}

int launch_logsoftmax_gather(const float* logits, int M, int V, int ldl, const int* cand, int k, float* out, hipStream_t s) {
    if (k < 1 || k > 256 || V > 16384) {
        cn_set_error("logsoftmax_gather: need 1 <= k <= 256 and V <= 16384");
        return -1;
    }
    if (M <= 0) return 0;
    hipLaunchKernelGGL(logsoftmax_gather_kernel, dim3(M), dim3(256), (size_t)V * sizeof(float), s, logits, V, ldl, cand, k, out);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Padding mask after 4x subsampling: src/tasks/cassnat_task.py:328 then embedding.py:121-122
// (mask[:, :, ::2][:, :, ::2]) => keymask[b][j] = feats[b][4j][0] != padding_idx.
// ---------------------------------------------------------------------------------------------
__global__ void keymask_kernel(const float* __restrict__ feats, int B, int T, int F, int Tp, int stride, float padding,
                               unsigned char* __restrict__ km) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Tp) return;
    const int b = i / Tp, j = i - b * Tp;
    const int t = stride * j;
    km[i] = (t < T && feats[((long long)b * T + t) * F] != padding) ? 1 : 0;
}

int launch_keymask(const float* feats, int B, int T, int F, int Tp, int stride, float padding, unsigned char* km,
                   hipStream_t s) {
    hipLaunchKernelGGL(keymask_kernel, dim3(cn_ceil_div(B * Tp, 256)), dim3(256), 0, s, feats, B, T, F, Tp, stride,
                       padding, km);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// The per-utterance records of a merged engine pass (kernels.h: UttMeta) from the pass's list of reference batches.
__global__ void expand_meta_kernel(SubList subs, UttMeta* __restrict__ meta, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int lo = 0, k = 0;
    for (; k < subs.n - 1 && b >= lo + subs.rows[k]; ++k) lo += subs.rows[k];
    const int T = subs.frames[k];
    const int T1 = (T - 1) / 2 + 1;
    UttMeta mrec;
    mrec.frames = T;
    mrec.tp = (T1 - 1) / 2 + 1;
    mrec.sub_lo = lo;
    mrec.sub_hi = lo + subs.rows[k];
    meta[b] = mrec;
}

int launch_expand_meta(const SubList& subs, UttMeta* meta, int B, hipStream_t s) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(expand_meta_kernel, dim3(cn_ceil_div(B, 256)), dim3(256), 0, s, subs, meta, B);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// extractor queries: pe[:ymax] repeated over the batch (src/models/cassnat.py:481)
__global__ void fill_queries_kernel(const float* __restrict__ table, float* __restrict__ out, int B, int U, int d) {
    const long long n4 = (long long)B * U * d / 4;
    const long long per = (long long)U * d / 4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
        reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(table)[i % per];
}

int launch_fill_queries(const float* table, float* out, int B, int U, int d, hipStream_t s) {
    const long long n4 = (long long)B * U * d / 4;
    if (n4 <= 0) return 0;
    hipLaunchKernelGGL(fill_queries_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, table, out, B, U, d);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// packed rows (launch_row_plan): one wave per row of the capacity; the row's utterance by bisection of row_off
__global__ __launch_bounds__(256) void fill_queries_packed_kernel(const float* __restrict__ table, float* __restrict__ out,
                                                                  const int* __restrict__ row_off, int B, int cap_rows, int d) {
    const int total = row_off[B];
    int end = (total + 127) & ~127;  // the row kernels' last 128-row block: finite rows behind the total
    if (end > cap_rows) end = cap_rows;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= end) return;
    int u = 0;
    if (row < total) {
        int lo = 0, hi = B;  // largest b with row_off[b] <= row (entries without rows share an offset: the last of them owns none)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (row_off[mid] <= row) lo = mid;
            else hi = mid;
        }
        u = row - row_off[lo];
    }
    const f32x4* src = reinterpret_cast<const f32x4*>(table + (long long)u * d);
    f32x4* dst = reinterpret_cast<f32x4*>(out + (long long)row * d);
    for (int i = lane; i < d / 4; i += 64) dst[i] = src[i];
}

int launch_fill_queries_packed(const float* table, float* out, const int* row_off, int B, int cap_rows, int d, hipStream_t s) {
    if (B <= 0 || cap_rows <= 0) return 0;
    hipLaunchKernelGGL(fill_queries_packed_kernel, dim3((unsigned)((cap_rows + 3) / 4)), dim3(256), 0, s, table, out, row_off, B,
                       cap_rows, d);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// use_unimask (src/models/cassnat.py:486-488): prepend a zero embedding, drop the last row
__global__ void shift_right_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int U, int d) {
    const long long n = (long long)B * U * d;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long u = (i / d) % U;
        y[i] = u == 0 ? 0.f : x[i - d];
    }
}

int launch_shift_right(const float* x, float* y, int B, int U, int d, hipStream_t s) {
    const long long n = (long long)B * U * d;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(shift_right_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, B, U, d);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
template <typename TD, typename TS>
__global__ void convert_kernel(const TS* __restrict__ src, TD* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = from_f32<TD>(to_f32(src[i]));
}

// flat fp32 <-> split-bf16 (n % 32 == 0: contiguous rows whose length is a multiple of 32)
__global__ void convert_to_split_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i);
        const float a[4] = {v[0], v[1], v[2], v[3]};
        bf16x4 hi, lo;
        cn_split4(a, hi, lo);
        unsigned char* d = dst + cn_split_off(4 * i);
        *reinterpret_cast<bf16x4*>(d) = hi;
        *reinterpret_cast<bf16x4*>(d + 64) = lo;
    }
}
__global__ void convert_from_split_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned char* p = src + cn_split_off(4 * i);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(p), lo = *reinterpret_cast<const bf16x4*>(p + 64);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)hi[j] + (float)lo[j];
        *reinterpret_cast<f32x4*>(dst + 4 * i) = o;
    }
}

static unsigned convert_grid(size_t n) {
    size_t g = (n + 255) / 256;
    return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

int launch_convert(int prec, const float* src, void* dst, size_t n, hipStream_t s) {
    if (n == 0) return 0;
    if (prec == CN_PREC_X3 && n % 32 != 0) {
        cn_set_error("convert: split-bf16 tensors hold a multiple of 32 elements");
        return -1;
    }
    if (prec == CN_PREC_F32)
        CN_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    else if (prec == CN_PREC_X3)
        hipLaunchKernelGGL(convert_to_split_kernel, dim3(convert_grid(n / 4)), dim3(256), 0, s, src, (unsigned char*)dst, n / 4);
    else
        hipLaunchKernelGGL((convert_kernel<bf16, float>), dim3(convert_grid(n)), dim3(256), 0, s, src, (bf16*)dst, n);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_convert_back(int prec, const void* src, float* dst, size_t n, hipStream_t s) {
    if (n == 0) return 0;
    if (prec == CN_PREC_X3 && n % 32 != 0) {
        cn_set_error("convert: split-bf16 tensors hold a multiple of 32 elements");
        return -1;
    }
    if (prec == CN_PREC_F32)
        CN_HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    else if (prec == CN_PREC_X3)
        hipLaunchKernelGGL(convert_from_split_kernel, dim3(convert_grid(n / 4)), dim3(256), 0, s, (const unsigned char*)src, dst,
                           n / 4);
    else
        hipLaunchKernelGGL((convert_kernel<float, bf16>), dim3(convert_grid(n)), dim3(256), 0, s, (const bf16*)src, dst,
                           n);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// rows of `width` 4-byte words from a [rows][src_ld] buffer into a [rows][dst_ld] one (a kernel, not hipMemcpy2DAsync: the
// runtime's pitched device-to-device copy takes a staging path of its own with occasional tens-of-milliseconds stalls)
__global__ void copy_rows_kernel(unsigned* __restrict__ dst, int dst_ld, const unsigned* __restrict__ src, int src_ld, int width,
                                 long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / width;
        const int c = (int)(i - r * width);
        dst[r * dst_ld + c] = src[r * src_ld + c];
    }
}
int launch_copy_rows(void* dst, int dst_ld, const void* src, int src_ld, int width, int rows, hipStream_t s) {
    const long long total = (long long)width * rows;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(convert_grid((size_t)total)), dim3(256), 0, s, (unsigned*)dst, dst_ld, (const unsigned*)src,
                       src_ld, width, total);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void fill_int_kernel(int* p, size_t n, int v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
int launch_fill_int(int* p, size_t n, int v, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(fill_int_kernel, dim3(convert_grid(n)), dim3(256), 0, s, p, n, v);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- ESA sampled alignment: label of frame i = second best iff its draw is 1 and exp(best log-prob) < threshold ----------
__global__ void esa_paths_kernel(const int* __restrict__ top2_idx, const float* __restrict__ top2_val,
                                 const unsigned char* __restrict__ select, float threshold, int* __restrict__ best, int M, int n) {
    // n paths per frame: best[g][i] for draw set g (select: [n][M], null = the best path)
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (long long)M * n) return;
    const int i = (int)(j % M);
    const int pick = (select && select[j] && expf(top2_val[2 * i]) < threshold) ? 1 : 0;
    best[j] = top2_idx[2 * i + pick];
}
int launch_esa_paths(const int* top2_idx, const float* top2_val, const unsigned char* select, float threshold, int* best, int M,
                     int n, hipStream_t s) {
    if (M <= 0 || n <= 0) return 0;
    hipLaunchKernelGGL(esa_paths_kernel, dim3((unsigned)(((long long)M * n + 255) / 256)), dim3(256), 0, s, top2_idx, top2_val, select,
                       threshold, best, M, n);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- TransformerLM input: x[b][u] = lut[tok[b][u]] * sqrt(d) + pe[u]   (embedding.py:71-78, 29-31) -----------------------
__global__ void lm_embed_kernel(const int* __restrict__ tok, int ld, const float* __restrict__ lut, const float* __restrict__ pe,
                                float* __restrict__ x, int B, int U, int d, float scale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * U * d) return;
    const int c = (int)(i % d);
    const long long bu = i / d;
    const int u = (int)(bu % U), b = (int)(bu / U);
    x[i] = lut[(long long)tok[(long long)b * ld + u] * d + c] * scale + pe[(long long)u * d + c];
}
int launch_lm_embed(const int* tok, int ld, const float* lut, const float* pe, float* x, int B, int U, int d, float scale,
                    hipStream_t s) {
    const long long n = (long long)B * U * d;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lm_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tok, ld, lut, pe, x, B, U, d, scale);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

__global__ void gather_logp_kernel(const float* __restrict__ logp, int V, const int* __restrict__ tgt, int ld,
                                   float* __restrict__ out, int B, int U) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * U) return;
    const int b = i / U, u = i - b * U;
    out[(long long)b * ld + u] = logp[(long long)i * V + tgt[(long long)b * ld + u]];
}
int launch_gather_logp(const float* logp, int V, const int* tgt, int ld, float* out, int B, int U, hipStream_t s) {
    if (B * U <= 0) return 0;
    hipLaunchKernelGGL(gather_logp_kernel, dim3(cn_ceil_div(B * U, 256)), dim3(256), 0, s, logp, V, tgt, ld, out, B, U);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// Global CMVN of a padded batch on the device: x[b][t][f] <- float((double(x) - mean[f]) / std[f]) for the frames t < len[b] of
// utterance b, later frames (collate's padding) untouched.  The reference does this per utterance on the host, in numpy's
// float64 with float64 statistics, and rounds to float32 when it collates (src/data/speech_loader.py:109-115, 147-149, 340): the
// same two IEEE operations and the same single rounding here, so the values are the reference's bit for bit - at HBM speed
// instead of the test-set loader's (which it was 3/4 of).
__global__ void cmvn_kernel(float* __restrict__ x, const int* __restrict__ len, const double* __restrict__ mean,
                            const double* __restrict__ sd, int T, int F) {
    const int b = blockIdx.y;
    const int lb = len[b];  // (clamped to the batch's frames: a bad length must not write past the utterance's rows)
    const long long n = (long long)(lb < 0 ? 0 : lb > T ? T : lb) * F;
    float* xb = x + (long long)b * T * F;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int f = (int)(i % F);
        xb[i] = (float)(((double)xb[i] - mean[f]) / sd[f]);
    }
}

// The reader's hand-over (SuperviseLoader.collate_fn, src/data/speech_loader.py:327-356, and the global CMVN of :109-115, 147-149) on
// the device: the utterances of an engine pass arrive PACKED - their archive rows back to back, exactly as they lie in the .ark, one
// DMA - and are spread over the padded batch here: out[r][t][:] = t < len[r] ? norm(packed[off[r] + t][:]) : pad, with
// norm(x) = float((double(x) - mean) / std) when statistics are given (the dataset's float64 arithmetic, one rounding: bit for
// bit) and x itself otherwise.  Replaces the host-side padded collate, the per-batch device copies and the separate CMVN pass.
// One workgroup per (utterance, 32-frame chunk); 16-byte accesses when F % 4 == 0.
__global__ __launch_bounds__(256) void unpack_rows_kernel(const float* __restrict__ packed, const int* __restrict__ off, const int* __restrict__ len,
                                                          float* __restrict__ out, int T, int F, float pad, const double* __restrict__ mean,
                                                          const double* __restrict__ sd) {
    const int r = blockIdx.y;
    const int n = len[r] < 0 ? 0 : (len[r] > T ? T : len[r]);
    const long long t0 = (long long)blockIdx.x * 32;
    if (t0 >= T) return;
    const int tn = (int)((T - t0) < 32 ? (T - t0) : 32);
    const float* src = packed + ((long long)off[r] + t0) * F;
    float* dst = out + ((long long)r * T + t0) * F;
    const int total = tn * F, valid = (int)((n - t0) <= 0 ? 0 : ((n - t0) < tn ? (n - t0) : tn)) * F;
    if ((F & 3) == 0 && (((size_t)src | (size_t)dst) & 15) == 0) {
        for (int i = 4 * threadIdx.x; i < total; i += 4 * 256) {
            f32x4 v = {pad, pad, pad, pad};
            if (i < valid) {  // (valid is a multiple of F, F of 4: a quad never straddles the utterance's end)
                v = *reinterpret_cast<const f32x4*>(src + i);
                if (mean) {
                    const int f = i % F;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (float)(((double)v[e] - mean[f + e]) / sd[f + e]);
                }
            }
            *reinterpret_cast<f32x4*>(dst + i) = v;
        }
    } else {
        for (int i = threadIdx.x; i < total; i += 256) {
            float v = pad;
            if (i < valid) {
                v = src[i];
                if (mean) v = (float)(((double)v - mean[i % F]) / sd[i % F]);
            }
            dst[i] = v;
        }
    }
}

int launch_unpack_rows(const float* packed, const int* off, const int* len, float* out, int rows, int T, int F, float pad,
                       const double* mean, const double* sd, hipStream_t s) {
    if (rows <= 0 || T <= 0 || F <= 0) return 0;
    if (rows > 65535) {
        cn_set_error("unpack_rows: more than 65535 utterances in one pass");
        return -1;
    }
    hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)cn_ceil_div(T, 32), (unsigned)rows), dim3(256), 0, s, packed, off, len, out, T, F,
                       pad, mean, sd);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the same hand-over for Kaldi COMPRESSED matrices (matrix/compressed-matrix.{h,cc}; data/kaldi_io.py restates the format) ----
// What `copy-feats --compress=true` and steps/make_fbank.sh write: one byte (or two) per value.  The utterances of a pass arrive as
// the archive holds them - each payload (16-byte global header: float min_value, float range, int32 num_rows, int32 num_cols; then
// the kind's data) at a 16-byte-aligned byte offset off[r] of the staging buffer - and are decompressed, normalised and padded here:
//   out[r][t][:] = t < len[r] ? norm(decompress(payload_r)[t][:]) : pad          (norm as in unpack_rows_kernel)
// Decompression is Kaldi's float32 arithmetic, every operation rounded on its own (its x86 builds have no fused multiply-add): the
// helpers uc_scale / uc_linear / uc_byte (feats_compress.h: the writer of these archives computes its quartiles with them) switch
// contraction off, since hipcc would otherwise fuse `a + b * c` and change the last bit of about one value in eleven of format 1's
// third segment.

// One workgroup per (utterance, 64-frame tile); the kind is uniform per workgroup.
// Format 1 (kind 1) is column-major - byte[c * num_rows + t] behind num_cols headers of four uint16 - with an arbitrary column
// stride, so a column's run starts at any byte.  The tile is 64 frames = one wavefront: a wave takes a column at a time, its lanes
// run along time, and one load instruction covers one contiguous 64-byte run of the column (at most two cache lines, no alignment
// needed for byte loads); a shorter tile would halve the run, a longer one only adds LDS.  The dequantised (and normalised) values
// go through LDS - [frame][column], row stride 97 floats: the column-wise writes hit 64 different banks - and leave row-major, 16
// bytes per store when F % 4 == 0.  Columns are walked in chunks of 96 (one chunk for 80- and 83-dimensional features).
// Formats 2 and 3 (uint16 / uint8, row-major) need no transpose.  Reads stay inside the payload its own header describes (which the
// host has checked against the bytes it staged): frames t < min(len[r], num_rows, T) only.
#define UC_TILE 64
#define UC_COLS 96
__global__ __launch_bounds__(256) void unpack_compressed_kernel(const unsigned char* __restrict__ staged, const int* __restrict__ off,
                                                                const int* __restrict__ len, const int* __restrict__ kind,
                                                                float* __restrict__ out, int T, int F, float pad,
                                                                const double* __restrict__ mean, const double* __restrict__ sd) {
    __shared__ float tile[UC_TILE][UC_COLS + 1];
    __shared__ float quart[UC_COLS][4];
    const int r = blockIdx.y;
    const long long t0 = (long long)blockIdx.x * UC_TILE;
    if (t0 >= T) return;
    const int tn = (int)((T - t0) < UC_TILE ? (T - t0) : UC_TILE);
    const unsigned char* p = staged + (long long)off[r];
    const float mn = *reinterpret_cast<const float*>(p), range = *reinterpret_cast<const float*>(p + 4);
    const int nr = *reinterpret_cast<const int*>(p + 8);
    const int k = kind[r];
    int n = len[r] < nr ? len[r] : nr;
    n = n < 0 ? 0 : (n > T ? T : n);
    if (k < 1 || k > 3) n = 0;
    const int valid = (int)((n - t0) <= 0 ? 0 : ((n - t0) < tn ? (n - t0) : tn));  // frames of this tile that hold data
    float* dst = out + ((long long)r * T + t0) * F;
    const bool quads = (F & 3) == 0 && ((size_t)dst & 15) == 0;
    if (k == 1) {
        const unsigned short* hdr = reinterpret_cast<const unsigned short*>(p + 16);
        const unsigned char* data = p + 16 + (long long)8 * F + t0;
        const float inc = uc_scale(range, 1.52590218966964e-05f);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int c0 = 0; c0 < F; c0 += UC_COLS) {
            const int cn = (F - c0) < UC_COLS ? (F - c0) : UC_COLS;
            if (valid > 0)
                for (int i = threadIdx.x; i < 4 * cn; i += 256) quart[i >> 2][i & 3] = uc_linear(mn, inc, hdr[4 * c0 + i]);
            __syncthreads();
            for (int c = wave; c < cn; c += 4) {
                float v = pad;
                if (lane < valid) {
                    v = uc_byte(quart[c][0], quart[c][1], quart[c][2], quart[c][3], data[(long long)(c0 + c) * nr + lane]);
                    if (mean) v = (float)(((double)v - mean[c0 + c]) / sd[c0 + c]);
                }
                tile[lane][c] = v;
            }
            __syncthreads();
            if (quads) {  // (cn is a multiple of 4: F and UC_COLS are)
                const int q = cn >> 2;
                for (int i = threadIdx.x; i < tn * q; i += 256) {
                    const int t = i / q, c = (i - t * q) * 4;
                    const f32x4 v = {tile[t][c], tile[t][c + 1], tile[t][c + 2], tile[t][c + 3]};
                    *reinterpret_cast<f32x4*>(dst + (long long)t * F + c0 + c) = v;
                }
            } else {
                for (int i = threadIdx.x; i < tn * cn; i += 256) {
                    const int t = i / cn, c = i - t * cn;
                    dst[(long long)t * F + c0 + c] = tile[t][c];
                }
            }
            __syncthreads();  // (the next chunk of columns overwrites the tile)
        }
        return;
    }
    // formats 2 (uint16) and 3 (uint8), row-major behind the 16-byte header (the payload starts on a 16-byte boundary: the uint16
    // are aligned)
    const float inc = uc_scale(range, k == 2 ? 1.52590218966964e-05f : (1 / 255.0f));
    const unsigned char* d8 = p + 16 + t0 * F;
    const unsigned short* d16 = reinterpret_cast<const unsigned short*>(p + 16) + t0 * F;
    const int total = tn * F, nvalid = valid * F;
    if (quads) {
        for (int i = 4 * threadIdx.x; i < total; i += 4 * 256) {
            f32x4 v = {pad, pad, pad, pad};
            if (i < nvalid) {  // (nvalid is a multiple of F, F of 4: a quad never straddles the utterance's end)
                const int f = i % F;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = uc_linear(mn, inc, k == 2 ? (unsigned)d16[i + e] : (unsigned)d8[i + e]);
                    if (mean) v[e] = (float)(((double)v[e] - mean[f + e]) / sd[f + e]);
                }
            }
            *reinterpret_cast<f32x4*>(dst + i) = v;
        }
    } else {
        for (int i = threadIdx.x; i < total; i += 256) {
            float v = pad;
            if (i < nvalid) {
                v = uc_linear(mn, inc, k == 2 ? (unsigned)d16[i] : (unsigned)d8[i]);
                if (mean) v = (float)(((double)v - mean[i % F]) / sd[i % F]);
            }
            dst[i] = v;
        }
    }
}

int launch_unpack_compressed(const unsigned char* staged, const int* off, const int* len, const int* kind, float* out, int rows, int T,
                             int F, float pad, const double* mean, const double* sd, hipStream_t s) {
    if (rows <= 0 || T <= 0 || F <= 0) return 0;
    if (rows > 65535) {
        cn_set_error("unpack_compressed: more than 65535 utterances in one pass");
        return -1;
    }
    hipLaunchKernelGGL(unpack_compressed_kernel, dim3((unsigned)cn_ceil_div(T, UC_TILE), (unsigned)rows), dim3(256), 0, s, staged, off,
                       len, kind, out, T, F, pad, mean, sd);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- frame splicing and skipping behind the same hand-over (src/data/speech_loader.py:141-158, src/data/feat_op.py:4-31) -----------
// The recipes' decode YAMLs read spliced frames (left_ctx 0, right_ctx 2, skip_frame 1: 240 values from 80).  Per utterance r with
// T = len[r] source rows of F0 values at row off[r]:
//   Tp    = skip > 1 ? T rounded up to a multiple of skip : T       (the dataset appends rows of literal zeros AFTER the CMVN)
//   n_out = skip > 1 ? Tp / skip : T                                 (clamped to T_out)
//   out[r][t][k * F0 + f] = pad                                      for t >= n_out, else with s = clamp(t * skip + k - left, 0, Tp - 1)
//                         = s < T ? norm(src[off[r] + s][f]) : 0.0f  (norm as in unpack_rows_kernel; edge rows are replicated - behind
//                                                                     appended zero rows the right edge replicates a ZERO row)
// One workgroup per (utterance, chunk of output frames).  The chunk's source span - (chunk - 1) * skip + left + right + 1 rows - is
// normalised into LDS once (the float64 divide runs per source element, not per copy of it); since block k of output frame i is span
// row i * skip + k, a whole output row is ONE contiguous window of (left + right + 1) * F0 floats of the span, starting at row
// i * skip.  Span rows that no output frame reads (skip > left + right + 1) are not staged.  Nothing at or behind row len[r] of an
// utterance is read: a padded source whose tail holds anything at all (the second calling form, off[r] = r * T0) is fine.
#define SP_CHUNK 32
#define SP_LDS_FLOATS 12288  // 48 KB: the span a workgroup may hold; the launcher shrinks the chunk to fit
#define SP_MAX_CTX 64        // left, right
#define SP_MAX_SKIP 64
__global__ __launch_bounds__(256) void splice_rows_kernel(const float* __restrict__ src, const int* __restrict__ off, const int* __restrict__ len,
                                                          float* __restrict__ out, int T_out, int F0, int left, int right, int sk, int chunk,
                                                          float pad, const double* __restrict__ mean, const double* __restrict__ sd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* span = reinterpret_cast<float*>(smem);
    const int r = blockIdx.y;
    const long long t0 = (long long)blockIdx.x * chunk;
    if (t0 >= T_out) return;
    const int tn = (int)((T_out - t0) < chunk ? (T_out - t0) : chunk);
    const int T = len[r] < 0 ? 0 : len[r];
    const long long Tp = sk > 1 ? ((long long)T + sk - 1) / sk * sk : (long long)T;
    long long n_out = Tp / sk;
    if (n_out > T_out) n_out = T_out;
    const int tv = (int)((n_out - t0) <= 0 ? 0 : ((n_out - t0) < tn ? (n_out - t0) : tn));  // output frames of this chunk that hold data
    const int ctx = left + right, W = (ctx + 1) * F0;
    const int span_rows = tv > 0 ? (tv - 1) * sk + ctx + 1 : 0;
    const long long lo = t0 * sk - left;  // source row of span row 0 (before clamping)
    const float* sb = src + (long long)off[r] * F0;
    float* dst = out + ((long long)r * T_out + t0) * W;
    const bool sparse = ctx + 1 < sk;  // span rows j with j % sk > ctx belong to no output frame
    if ((F0 & 3) == 0 && (((size_t)sb | (size_t)dst) & 15) == 0) {
        const int q = F0 >> 2;
        for (int idx = threadIdx.x; idx < span_rows * q; idx += 256) {
            const int j = idx / q, c = (idx - j * q) * 4;
            if (sparse && (j % sk) > ctx) continue;
            long long s = lo + j;
            s = s < 0 ? 0 : (s > Tp - 1 ? Tp - 1 : s);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (s < T) {
                v = *reinterpret_cast<const f32x4*>(sb + s * F0 + c);
                if (mean) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (float)(((double)v[e] - mean[c + e]) / sd[c + e]);
                }
            }
            *reinterpret_cast<f32x4*>(span + j * F0 + c) = v;
        }
        __syncthreads();
        const int wq = W >> 2;
        for (int idx = threadIdx.x; idx < tn * wq; idx += 256) {
            const int i = idx / wq, c = (idx - i * wq) * 4;
            f32x4 v = {pad, pad, pad, pad};
            if (i < tv) v = *reinterpret_cast<const f32x4*>(span + i * sk * F0 + c);
            *reinterpret_cast<f32x4*>(dst + (long long)i * W + c) = v;
        }
    } else {
        for (int idx = threadIdx.x; idx < span_rows * F0; idx += 256) {
            const int j = idx / F0, c = idx - j * F0;
            if (sparse && (j % sk) > ctx) continue;
            long long s = lo + j;
            s = s < 0 ? 0 : (s > Tp - 1 ? Tp - 1 : s);
            float v = 0.f;
            if (s < T) {
                v = sb[s * F0 + c];
                if (mean) v = (float)(((double)v - mean[c]) / sd[c]);
            }
            span[idx] = v;
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < tn * W; idx += 256) {
            const int i = idx / W, c = idx - i * W;
            dst[idx] = i < tv ? span[i * sk * F0 + c] : pad;
        }
    }
}

int launch_splice_rows(const float* src, const int* off, const int* len, float* out, int rows, int T_out, int F0, int left, int right,
                       int skip, float pad, const double* mean, const double* sd, hipStream_t s) {
    if (rows <= 0 || T_out <= 0 || F0 <= 0) {
        cn_set_error("splice_rows: rows, T_out and F0 must be positive");
        return -1;
    }
    if (left < 0 || right < 0 || skip < 0 || left > SP_MAX_CTX || right > SP_MAX_CTX || skip > SP_MAX_SKIP) {
        cn_set_error("splice_rows: need 0 <= left, right <= 64 and 0 <= skip <= 64");
        return -1;
    }
    if (rows > 65535) {
        cn_set_error("splice_rows: more than 65535 utterances in one pass");
        return -1;
    }
    const int sk = skip < 1 ? 1 : skip;  // (skip_feat: 0 and 1 both keep every frame)
    const long long W = (long long)(left + right + 1) * F0;
    if (W > SP_LDS_FLOATS) {
        cn_set_error("splice_rows: a spliced row of more than 12288 values does not fit the kernel's LDS");
        return -1;
    }
    if ((long long)rows * T_out * W > 0x7fffffffLL || (long long)T_out * sk > 0x7fffffffLL) {
        cn_set_error("splice_rows: the batch (rows x T_out x spliced width) overflows 32-bit indexing");
        return -1;
    }
    // the largest chunk of output frames whose source span fits the LDS (32 for the recipes' shapes; 1 always fits: W floats)
    int chunk = SP_CHUNK;
    while (chunk > 1 && ((long long)(chunk - 1) * sk + left + right + 1) * F0 > SP_LDS_FLOATS) --chunk;
    const size_t lds = (size_t)((chunk - 1) * sk + left + right + 1) * F0 * sizeof(float);
    hipLaunchKernelGGL(splice_rows_kernel, dim3((unsigned)cn_ceil_div(T_out, chunk), (unsigned)rows), dim3(256), lds, s, src, off, len, out,
                       T_out, F0, left, right, sk, chunk, pad, mean, sd);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_cmvn(float* x, const int* len, const double* mean, const double* sd, int B, int T, int F, hipStream_t s) {
    if (B <= 0 || T <= 0 || F <= 0) return 0;
    const int per = cn_ceil_div(T * F, 256);
    hipLaunchKernelGGL(cmvn_kernel, dim3((unsigned)(per < 64 ? per : 64), (unsigned)B), dim3(256), 0, s, x, len, mean, sd, T, F);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- fp16 engine: the features against the range its half-precision operands hold (model.hip: op16_feat_limit) -------------------
__global__ __launch_bounds__(256) void feature_range_kernel(const float* __restrict__ x, size_t n4, size_t n, const float* __restrict__ limit,
                                                            unsigned int* fault) {
    const float lim = *limit;
    if (!(lim > 0.f)) return;
    float m = 0.f;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 v = x4[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    // what the 16-byte loads did not cover: the last n % 4 values - or everything, for a batch that does not start on a 16-byte
    // boundary (a view into a larger tensor with an odd feature width)
    for (size_t i = 4 * n4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    if (m > lim) *fault = 1u;  // (racing writers store the same word; page-locked host memory, read after the stream has drained)
}

int launch_feature_range(const float* x, size_t n, const float* limit, unsigned int* fault, hipStream_t s) {
    if (n == 0) return 0;
    const size_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) ? 0 : n / 4;
    const int grid = (int)std::min<size_t>(2048, ((n4 ? n4 : n) + 255) / 256 + 1);
    hipLaunchKernelGGL(feature_range_kernel, dim3(grid), dim3(256), 0, s, x, n4, n, limit, fault);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}
