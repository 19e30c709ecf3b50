// AST beam search with word n-gram shallow fusion for gfx950: `--task art`, `decode_type: ctc_att`, `rank_model: n-gram`, an ARPA
// model and lm_weight > 0.  The reference fuses only a TransformerLM there; this is the word-level fusion of ctc_ngram_search.h in
// Transformer.beam_decode's step loop.  ast_ngram_search.h holds the step functions, include/cassnat_hip_ast_ngram.h the contract.
//
// What a candidate token adds depends on its class alone - eos, a piece that begins a word, any other - so a step needs two floats
// per beam slot (adds) and the vocabulary's piece_starts.  ast_ngram_adds_kernel recomputes them from the slot's own token row every
// step, one wave per slot, with no state that follows the beam:
//   * lanes take the row's ids 64 at a time; the segmented scan over the piece monoid and the ordered compaction of the closed words'
//     ids are ngram_score_kernel's (ngram.hip), but the words are not scored: only the last NG_HIST ids and their count are kept;
//   * the up to 15 + 15 table probes of score(open word | history) and score(</s> | history [+ open word]) go to lanes 0 .. 31 and
//     lane 0 adds them up in ng_word_score's float32 order;
//   * when the step has its candidates already (with CTC: the attention top-K), lanes write their terms in the same launch.
// Every probe loop is bounded by its table's slot count; ids outside [0, vocab) and ids equal to eos contribute no piece; a row's
// length is clamped to its stride.
#include "ast_ngram_search.h"
#include "kernels.h"

__device__ __forceinline__ uint64_t an_shfl_up(uint64_t v, int delta) {
    const unsigned lo = __shfl_up((unsigned)v, delta, 64), hi = __shfl_up((unsigned)(v >> 32), delta, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t an_shfl(uint64_t v, int lane) {
    const unsigned lo = __shfl((unsigned)v, lane, 64), hi = __shfl((unsigned)(v >> 32), lane, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ NgPiece an_shfl_up(const NgPiece& v, int delta) {
    NgPiece r;
    r.h = an_shfl_up(v.h, delta), r.pw = an_shfl_up(v.pw, delta), r.starts = __shfl_up(v.starts, delta, 64);
    return r;
}

__global__ __launch_bounds__(64) void ast_ngram_adds_kernel(cn_ngram_desc d, const int32_t* __restrict__ tok, int ld, int col0,
                                                            const int32_t* __restrict__ len, int len_bias, int32_t eos,
                                                            float* __restrict__ adds, const int32_t* __restrict__ idx, int K,
                                                            float* __restrict__ term) {
    __shared__ int32_t ids[NG_HIST + 64];  // the last NG_HIST ids of the chunks before, then this chunk's closed words in order
    __shared__ AnState st;
    __shared__ NgProbe pr[2 * NG_TASKS];
    __shared__ float out[2];
    const int row = blockIdx.x, lane = threadIdx.x;
    int n = len[row] + len_bias;
    n = n < 0 ? 0 : (n > ld - col0 ? ld - col0 : n);
    const int32_t* t_row = tok + (long long)row * ld + col0;
    if (lane < NG_HIST) ids[lane] = d.bos;
    __syncthreads();
    int nwords = 0;  // (uniform over the wave, as is carry)
    NgPiece carry = ng_piece(d, 0, false);
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const int32_t t = i < n ? t_row[i] : eos;
        const bool real = i < n && an_real(d, t, eos);
        NgPiece v = ng_piece(d, t, real);
        const bool starts = real && v.starts;
        for (int delta = 1; delta < 64; delta <<= 1) {
            const NgPiece a = an_shfl_up(v, delta);
            if (lane >= delta) v = ng_combine(a, v);
        }
        const NgPiece inc = ng_combine(carry, v);
        NgPiece ex = an_shfl_up(inc, 1);
        if (lane == 0) ex = carry;
        const bool emit = starts && ex.pw != 1;  // this piece begins a word: the one before it, if there is one, is complete
        const int32_t id = emit ? ng_word_id(d, ex.h) : 0;
        const unsigned long long ball = __ballot(emit);
        if (emit) ids[NG_HIST + __popcll(ball & ((1ull << lane) - 1ull))] = id;
        carry.h = an_shfl(inc.h, 63), carry.pw = an_shfl(inc.pw, 63), carry.starts = __shfl(inc.starts, 63, 64);
        __syncthreads();
        const int m = __popcll(ball);
        const int32_t keep = lane < NG_HIST ? ids[m + lane] : 0;
        __syncthreads();
        if (lane < NG_HIST) ids[lane] = keep;
        nwords += m;
        __syncthreads();
    }
    if (lane < NG_HIST) st.hist[lane] = ids[lane];
    if (lane == 0) {
        st.carry = carry;
        st.nwords = nwords;
        st.hist[NG_HIST] = carry.pw != 1 ? ng_word_id(d, carry.h) : d.bos;
        st.hist[NG_HIST + 1] = d.bos;
    }
    __syncthreads();
    if (lane < 2 * NG_TASKS) an_probe(d, st, lane, &pr[lane]);
    __syncthreads();
    if (lane == 0) {
        an_adds(d, st, pr, out);
        adds[2 * (long long)row] = out[0];
        adds[2 * (long long)row + 1] = out[1];
    }
    if (!term) return;
    __syncthreads();
    for (int c = lane; c < K; c += 64) term[(long long)row * K + c] = an_term(d.piece_starts, out, eos, idx[(long long)row * K + c], d.vocab);
}

__global__ __launch_bounds__(256) void ast_ngram_terms_kernel(const unsigned char* __restrict__ starts, const float* __restrict__ adds,
                                                              int32_t eos, const int32_t* __restrict__ idx, long long total, int K,
                                                              float* __restrict__ term) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    // (the ids are a top-k's: below the vocabulary `starts` covers; a negative one is no piece)
    term[i] = an_term(starts, adds + 2 * (i / K), eos, idx[i], 0x7fffffff);
}

int launch_ast_ngram_adds(const cn_ngram_desc& d, const int* tok, int ld, int col0, const int* len, int len_bias, int n, int eos,
                          float* adds, const int* idx, int K, float* term, hipStream_t s) {
    const std::string bad = ng_check_desc(d);
    if (!bad.empty()) {
        cn_set_error("ast_ngram_adds: " + bad);
        return -1;
    }
    if (!tok || !len || !adds || n < 1 || ld < 1 || col0 < 0 || col0 > ld || (term && (!idx || K < 1))) {
        cn_set_error("ast_ngram_adds: null argument, or rows / stride < 1");
        return -1;
    }
    hipLaunchKernelGGL(ast_ngram_adds_kernel, dim3((unsigned)n), dim3(64), 0, s, d, tok, ld, col0, len, len_bias, eos, adds, idx, K, term);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ast_ngram_terms(const unsigned char* starts, const float* adds, int eos, const int* idx, int n, int K, float* term,
                           hipStream_t s) {
    if (!starts || !adds || !idx || !term || n < 1 || K < 1) {
        cn_set_error("ast_ngram_terms: null argument, or rows / K < 1");
        return -1;
    }
    const long long total = (long long)n * K;
    hipLaunchKernelGGL(ast_ngram_terms_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, starts, adds, eos, idx, total, K, term);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int cn_op_ast_ngram_adds(const cn_ngram_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n, int32_t eos,
                                    float* adds, void* stream) {
    if (!desc) {
        cn_set_error("cn_op_ast_ngram_adds: null argument");
        return -1;
    }
    return launch_ast_ngram_adds(*desc, tok, ld, 0, len, 0, n, eos, adds, nullptr, 0, nullptr, (hipStream_t)stream);
}

// the same step functions on the host: every pointer a host pointer, no GPU call
extern "C" int cn_ast_ngram_adds_host(const cn_ngram_desc* desc, const int32_t* tok, int32_t ld, const int32_t* len, int32_t n, int32_t eos,
                                      float* adds) {
    if (!desc || !tok || !len || !adds || n < 1 || ld < 1) {
        cn_set_error("cn_ast_ngram_adds_host: null argument, or rows / stride < 1");
        return -1;
    }
    const std::string bad = ng_check_desc(*desc);
    if (!bad.empty()) {
        cn_set_error("cn_ast_ngram_adds_host: " + bad);
        return -1;
    }
    for (int32_t r = 0; r < n; ++r) {
        const int m = len[r] < 0 ? 0 : (len[r] > ld ? ld : len[r]);
        an_adds_row_host(*desc, tok + (long long)r * ld, m, eos, adds + 2 * (long long)r);
    }
    return 0;
}

extern "C" int cn_op_ast_ngram_terms(const uint8_t* starts, const float* adds, int32_t eos, const int32_t* idx, int32_t n, int32_t K,
                                     float* term, void* stream) {
    return launch_ast_ngram_terms(starts, adds, eos, idx, n, K, term, (hipStream_t)stream);
}

extern "C" int cn_op_logsoftmax_class_topk(const float* att, int32_t M, int32_t V, float temperature, const uint8_t* starts, const float* adds,
                                           int32_t eos, float w, int32_t k, int32_t* idx, float* val, void* stream) {
    if (!att || !starts || !adds || !idx || !val || M < 1 || V < 1 || !(temperature > 0.f)) {
        cn_set_error("cn_op_logsoftmax_class_topk: bad argument");
        return -1;
    }
    return launch_logsoftmax_class_topk(att, M, V, V, temperature, starts, adds, eos, w, k, idx, val, (hipStream_t)stream);
}
