// Weighted edit alignment of id sequences for gfx950: the device half of the scorer (decode_asr --hip_score, bin/score_asr).
// edit_align_search.h holds the step functions, include/cassnat_hip_score.h the contract.
//
// One workgroup of one wave per pair, the rows of the table in order, everything of the row loop in LDS:
//   * the two live rows of H + 1 int32 and the hyp ids, position j with lane j % 64 (consecutive dwords: no bank conflict);
//   * a row is one pass over chunks of 64 positions: the candidates that do not depend on the row (diagonal, up), a prefix minimum
//     of t[j] - c_ins * j over the wave (six shuffle steps), the minimum so far carried from chunk to chunk in a register;
//   * the ref ids come 64 at a time into one register per lane and reach a row by a lane read, so the row loop reads no global memory;
//   * the moves, 2 bits per cell: two __ballot masks per (row, chunk), written by lane 0.  In the scratch form (a table too large for
//     the LDS, or the caller's threshold) the same two words go to global memory instead.
//   One barrier per row (of a single wave: it orders the LDS traffic, nothing waits).
// The walk back is serial by nature: lane 0 follows the masks, a counted loop of at most R + H steps, and leaves the codes backwards in
// LDS; all lanes then store them forwards.  A span that leaves its buffer ends the pair before anything is read through it; R and H
// are clamped; every barrier is reached by the whole wave (R, H and the span check are uniform over it).
#include "edit_align_search.h"
#include "kernels.h"

template <bool BP_LDS>
__global__ __launch_bounds__(EA_THREADS) void edit_align_kernel(EditArgs a, int row_words, int lds_fixed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = blockIdx.x, lane = threadIdx.x;
    int* prev = reinterpret_cast<int*>(smem);  // [row_words]
    int* cur = prev + row_words;               // [row_words]
    int* hypl = cur + row_words;               // [row_words]
    uint8_t* back = reinterpret_cast<uint8_t*>(hypl + row_words);  // [max_ref + max_hyp]
    const int R = ea_clamp(a.ref_len[n], 0, a.max_ref), H = ea_clamp(a.hyp_len[n], 0, a.max_hyp), chunks = ea_chunks(H + 1);
    const int64_t rb = a.ref_begin[n], hb = a.hyp_begin[n], ob = a.ops_begin[n];
    if (!ea_span_ok(a, rb, hb, ob, R, H)) {  // (uniform: the whole wave leaves)
        if (lane < 4) a.counts[(size_t)n * 4 + lane] = 0;
        if (lane == 0) {
            a.cost[n] = -1;
            a.path_len[n] = 0;
        }
        return;
    }
    unsigned long long* bp;
    if constexpr (BP_LDS)
        bp = reinterpret_cast<unsigned long long*>(smem + lds_fixed);
    else
        bp = a.bp + (size_t)n * a.max_ref * ea_chunks(a.max_hyp + 1) * 2;  // (R <= max_ref rows of chunks <= ea_chunks(max_hyp + 1))
    const int32_t* ref = a.ref + rb;
    const int32_t* hyp = a.hyp + hb;
    const int c_sub = a.c_sub, c_ins = a.c_ins, c_del = a.c_del;

    for (int j = lane; j <= H; j += EA_THREADS) {
        prev[j] = j * c_ins;
        if (j < H) hypl[j] = hyp[j];
    }
    __syncthreads();
    int32_t rreg = 0;
    for (int i = 1; i <= R; ++i) {
        if (((i - 1) & 63) == 0) rreg = i - 1 + lane < R ? ref[i - 1 + lane] : 0;
        const int32_t r = __shfl(rreg, (i - 1) & 63);
        int carry = INT_MAX;
        for (int base = 0; base <= H; base += EA_THREADS) {  // (uniform over the wave: every lane reaches the shuffles and ballots)
            const int j = base + lane;
            const bool live = j <= H;
            int diag = 0, up = 0, v = INT_MAX;
            bool eq = false;
            if (live) {
                int t = i * c_del;
                if (j > 0) {
                    eq = hypl[j - 1] == r;
                    ea_cand(prev[j - 1], prev[j], eq, c_sub, c_del, &diag, &up);
                    t = diag < up ? diag : up;
                }
                v = t - c_ins * j;
            }
#pragma unroll
            for (int d = 1; d < EA_THREADS; d <<= 1) {
                const int o = __shfl_up(v, d);
                if (lane >= d && o < v) v = o;
            }
            if (carry < v) v = carry;
            carry = __shfl(v, EA_THREADS - 1);
            int mv = 0;
            if (live) {
                const int dd = v + c_ins * j;
                cur[j] = dd;
                mv = ea_move(dd, diag, up, eq, j == 0);
            }
            const unsigned long long lo = __ballot(mv & 1), hi = __ballot(mv & 2);
            if (lane == 0) {
                unsigned long long* w = bp + ((size_t)(i - 1) * chunks + (base >> 6)) * 2;
                w[0] = lo;
                w[1] = hi;
            }
        }
        __syncthreads();
        int* x = prev;
        prev = cur;
        cur = x;
    }
    // prev: row R.  (the barrier behind the last row has also made the scratch form's masks visible to the walk)
    const int cost = prev[H];
    int c4[4] = {0, 0, 0, 0};
    int P = 0;
    if (lane == 0) P = ea_walk(bp, chunks, R, H, back, c4);
    __syncthreads();
    P = __shfl(P, 0);
    uint8_t* ops = a.ops + ob;
    for (int k = lane; k < P; k += EA_THREADS) ops[k] = back[P - 1 - k];
    if (lane == 0) {
        a.cost[n] = cost;
        a.path_len[n] = P;
        for (int k = 0; k < 4; ++k) a.counts[(size_t)n * 4 + k] = c4[k];
    }
}

template <bool BP_LDS>
static int launch_edit(const EditArgs& a, hipStream_t s) {
    static CnAttrOnce attr_once;  // (one per instantiation)
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        CN_HIP_CHECK(hipFuncSetAttribute((const void*)edit_align_kernel<BP_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EA_LDS_CAP));
        attr_once.mark(attr_dev);
    }
    const size_t fixed = ea_lds_fixed(a.max_ref, a.max_hyp), lds = fixed + (BP_LDS ? ea_bp_bytes(a.max_ref, a.max_hyp) : 0);
    hipLaunchKernelGGL(edit_align_kernel<BP_LDS>, dim3((unsigned)a.N), dim3(EA_THREADS), lds, s, a, (int)ea_row_words(a.max_hyp), (int)fixed);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_edit_align(const EditArgs& a, long long bp_lds_limit, hipStream_t s) {
    const std::string bad = ea_check(a);
    if (!bad.empty()) {
        cn_set_error("edit_align: " + bad);
        return -1;
    }
    if (ea_bp_in_lds(a.max_ref, a.max_hyp, bp_lds_limit)) return launch_edit<true>(a, s);
    if (!a.bp && ea_scratch_bytes(a.N, a.max_ref, a.max_hyp, bp_lds_limit) > 0) {
        cn_set_error("edit_align: the scratch form needs its back-pointer buffer");
        return -1;
    }
    return launch_edit<false>(a, s);
}

// the same step functions on the host: every pointer a host pointer, no GPU call
extern "C" int cn_edit_align_host(const int32_t* ref, int64_t ref_total, const int64_t* ref_begin, const int32_t* ref_len, const int32_t* hyp,
                                  int64_t hyp_total, const int64_t* hyp_begin, const int32_t* hyp_len, int32_t N, int32_t max_ref,
                                  int32_t max_hyp, int32_t c_sub, int32_t c_ins, int32_t c_del, int32_t* cost, int32_t* counts,
                                  int32_t* path_len, uint8_t* ops, int64_t ops_total, const int64_t* ops_begin) {
    EditArgs a;
    a.ref = ref, a.ref_begin = ref_begin, a.ref_len = ref_len, a.hyp = hyp, a.hyp_begin = hyp_begin, a.hyp_len = hyp_len;
    a.ops_begin = ops_begin, a.ref_total = ref_total, a.hyp_total = hyp_total, a.ops_total = ops_total;
    a.N = N, a.max_ref = max_ref, a.max_hyp = max_hyp, a.c_sub = c_sub, a.c_ins = c_ins, a.c_del = c_del;
    a.cost = cost, a.counts = counts, a.path_len = path_len, a.ops = ops;
    std::string bad;
    if (ea_run_host(a, &bad) != 0) {
        cn_set_error("cn_edit_align_host: " + bad);
        return -1;
    }
    return 0;
}
