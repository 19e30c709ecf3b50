// AST beam search with contextual phrase biasing for gfx950: `--task art`, `decode_type: ctc_att`, `--hip_bias FILE --hip_bias_search
// att`.  The reference has no biasing; this is the phrase automaton of the CTC prefix beam search (ctc_bias_search.h) in
// Transformer.beam_decode's step loop.  ast_bias_search.h holds the step functions, include/cassnat_hip_ast_bias.h the contract.
//
// What a candidate token adds depends on the hypothesis' node AND on the token, so a step needs a node per beam slot and a walk over
// the hashed edges per candidate:
//   * ast_bias_nodes_kernel folds a token row into its node, one lane per row (a serial chain of dependent loads: the stateless entry
//     of the caller-managed loop and of the tests; cn_decode_ast does not launch it);
//   * ast_bias_terms_kernel gives the terms at the K candidates of a row, one thread per (row, candidate);
//   * logsoftmax_bias_topk_kernel, logsoftmax_class_topk_kernel's sibling (rowops.hip), ranks the whole vocabulary with the terms:
//     the row's failure chain and its node's value go to LDS once per workgroup, every entry then probes the chain's nodes in order -
//     at the root, the common case, one probe per entry.
// Inside cn_decode_ast the last two take the slot's node from the step before through the ancestor table (AbCarry) and write this
// step's: one cb_step per slot and step, no launch of its own.  Every probe loop is bounded by its table's slot count, the failure
// walk by 32; a child or failure target outside the node table counts as the root.
#include "ast_bias_search.h"
#include "kernels.h"
#include "rowreduce.h"

__global__ __launch_bounds__(64) void ast_bias_nodes_kernel(cn_bias_desc d, const int32_t* __restrict__ tok, int ld,
                                                            const int32_t* __restrict__ len, int n, int32_t* __restrict__ node_out) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;
    int m = len[row];
    m = m < 0 ? 0 : (m > ld ? ld : m);
    node_out[row] = ab_fold(d, tok + (long long)row * ld, m);
}

__global__ __launch_bounds__(256) void ast_bias_terms_kernel(cn_bias_desc d, const int32_t* __restrict__ node, AbCarry cs, int32_t eos,
                                                             const int32_t* __restrict__ idx, long long total, int K,
                                                             float* __restrict__ term) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int row = (int)(i / K);
    int nd;
    if (cs.out) {  // (the K threads of a row read the same words; the first of them keeps the node for the next step)
        nd = ab_carried(d, cs, row);
        if (i - (long long)row * K == 0) cs.out[row] = nd;
    } else {
        nd = node[row];
    }
    // (the ids are a top-k's: below the vocabulary; a negative one is no piece)
    term[i] = ab_term(d, nd, eos, 0x7fffffff, idx[i]);
}

// Phrase biasing without CTC (include/cassnat_hip_ast_bias.h).  The row arithmetic before the add - x / T, maximum, log-sum-exp,
// (x - max) - lse - and the selection after it are logsoftmax_topk_kernel's, so terms that are all +0.0f give its output bit for bit.
__global__ __launch_bounds__(256) void logsoftmax_bias_topk_kernel(const float* __restrict__ logits, int V, int ldl, float temperature,
                                                                   int k, int* __restrict__ idx, float* __restrict__ val, cn_bias_desc d,
                                                                   const int32_t* __restrict__ node, AbCarry cs, int eos) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ RowReduceLds red;
    __shared__ int32_t chain[AB_CHAIN];
    __shared__ int chain_n;
    __shared__ float chain_v;
    const float* p = logits + (long long)blockIdx.x * ldl;
    const int tid = threadIdx.x;
    if (tid == 0) {  // (the barriers of the reductions below stand between this and the readers)
        int nd = cs.out ? ab_carried(d, cs, blockIdx.x) : ab_node(d, node[blockIdx.x]);
        if (cs.out) cs.out[blockIdx.x] = nd;
        if (d.nodes <= 1) {
            chain[0] = 0, chain_n = 0, chain_v = 0.f;
        } else {
            chain_n = ab_chain(d, nd, chain);
            chain_v = nd != 0 ? d.value[nd] : 0.f;
        }
    }
    if (temperature != 1.0f)
        for (int i = tid; i < V; i += 256) row[i] = p[i] / temperature;
    else
        for (int i = tid; i < V; i += 256) row[i] = p[i];
    float rmax;
    int rarg;
    rr_local_best(row, V, tid, rmax, rarg);
    rr_block_argmax(red, tid, rmax, rarg);
    const float lse = rr_block_lse(red, row, V, tid, rmax);
    const int m = chain_n;
    const float vn = chain_v;
    if (m == 0) {
        for (int i = tid; i < V; i += 256) row[i] = __fadd_rn(__fsub_rn(__fsub_rn(row[i], rmax), lse), 0.f);
    } else {
        for (int i = tid; i < V; i += 256)
            row[i] = __fadd_rn(__fsub_rn(__fsub_rn(row[i], rmax), lse), ab_term_chain(d, chain, m, vn, eos, V, i));
    }
    rr_select_rounds(red, row, V, tid, k, -INFINITY, [&](int r, int bidx, float best) {
        idx[(long long)blockIdx.x * k + r] = bidx;
        val[(long long)blockIdx.x * k + r] = best;
    });
}

namespace {
int bias_desc_ok(const char* who, const cn_bias_desc& d) {
    const std::string bad = cb_check_desc(d);
    if (bad.empty()) return 0;
    cn_set_error(std::string(who) + ": " + bad);
    return -1;
}
}  // namespace

int launch_ast_bias_nodes(const cn_bias_desc& d, const int* tok, int ld, const int* len, int n, int* node_out, hipStream_t s) {
    CN_TRY(bias_desc_ok("ast_bias_nodes", d));
    if (!tok || !len || !node_out || n < 1 || ld < 1) {
        cn_set_error("ast_bias_nodes: null argument, or rows / stride < 1");
        return -1;
    }
    hipLaunchKernelGGL(ast_bias_nodes_kernel, dim3((unsigned)cn_ceil_div(n, 64)), dim3(64), 0, s, d, tok, ld, len, n, node_out);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ast_bias_terms(const cn_bias_desc& d, const int* node, const AbCarry& cs, int eos, const int* idx, int n, int K, float* term,
                          hipStream_t s) {
    CN_TRY(bias_desc_ok("ast_bias_terms", d));
    if ((!node && !cs.out) || !idx || !term || n < 1 || K < 1) {
        cn_set_error("ast_bias_terms: null argument, or rows / K < 1");
        return -1;
    }
    const long long total = (long long)n * K;
    hipLaunchKernelGGL(ast_bias_terms_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d, node, cs, eos, idx, total, K, term);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_logsoftmax_bias_topk(const float* att, int M, int V, int ldl, float temperature, const cn_bias_desc& d, const int* node,
                                const AbCarry& cs, int eos, int k, int* idx, float* val, hipStream_t s) {
    CN_TRY(bias_desc_ok("logsoftmax_bias_topk", d));
    if (k < 1 || k > 32 || k > V || V > 8192) {
        cn_set_error("logsoftmax_bias_topk: need 1 <= k <= min(32, V) and V <= 8192");
        return -1;
    }
    if (M <= 0) return 0;
    hipLaunchKernelGGL(logsoftmax_bias_topk_kernel, dim3(M), dim3(256), (size_t)V * sizeof(float), s, att, V, ldl, temperature, k, idx, val,
                       d, node, cs, eos);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int cn_op_ast_bias_nodes(const cn_bias_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n,
                                    int32_t* node_out, void* stream) {
    if (!desc) {
        cn_set_error("cn_op_ast_bias_nodes: null argument");
        return -1;
    }
    return launch_ast_bias_nodes(*desc, tok, ld, len, n, node_out, (hipStream_t)stream);
}

// the same step functions on the host: every pointer a host pointer, no GPU call
extern "C" int cn_ast_bias_nodes_host(const cn_bias_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n,
                                      int32_t* node_out) {
    if (!desc || !tok || !len || !node_out || n < 1 || ld < 1) {
        cn_set_error("cn_ast_bias_nodes_host: null argument, or rows / stride < 1");
        return -1;
    }
    CN_TRY(bias_desc_ok("cn_ast_bias_nodes_host", *desc));
    for (int32_t r = 0; r < n; ++r) {
        const int m = len[r] < 0 ? 0 : (len[r] > ld ? ld : len[r]);
        node_out[r] = ab_fold(*desc, tok + (long long)r * ld, m);
    }
    return 0;
}

extern "C" int cn_op_ast_bias_terms(const cn_bias_desc* desc, const int32_t* node, int32_t eos, const int32_t* idx, int32_t n, int32_t K,
                                    float* term, void* stream) {
    if (!desc || !node) {
        cn_set_error("cn_op_ast_bias_terms: null argument");
        return -1;
    }
    return launch_ast_bias_terms(*desc, node, AbCarry{}, eos, idx, n, K, term, (hipStream_t)stream);
}

extern "C" int cn_ast_bias_terms_host(const cn_bias_desc* desc, const int32_t* node, int32_t eos, const int32_t* idx, int32_t n, int32_t K,
                                      float* term) {
    if (!desc || !node || !idx || !term || n < 1 || K < 1) {
        cn_set_error("cn_ast_bias_terms_host: null argument, or rows / K < 1");
        return -1;
    }
    CN_TRY(bias_desc_ok("cn_ast_bias_terms_host", *desc));
    for (long long i = 0; i < (long long)n * K; ++i) term[i] = ab_term(*desc, node[i / K], eos, 0x7fffffff, idx[i]);
    return 0;
}

extern "C" int cn_op_logsoftmax_bias_topk(const float* att, int32_t M, int32_t V, float temperature, const cn_bias_desc* desc,
                                          const int32_t* node, int32_t eos, int32_t k, int32_t* idx, float* val, void* stream) {
    if (!att || !desc || !node || !idx || !val || M < 1 || V < 1 || !(temperature > 0.f)) {
        cn_set_error("cn_op_logsoftmax_bias_topk: bad argument");
        return -1;
    }
    return launch_logsoftmax_bias_topk(att, M, V, V, temperature, *desc, node, AbCarry{}, eos, k, idx, val, (hipStream_t)stream);
}
