// Reductions of one row by one 256-thread (four-wave) workgroup: the generator tails of rowops.hip and the fused row kernel of
// natlm.hip are built from these and from nothing else, which is what keeps them equal to each other bit for bit.  Thread tid owns
// entries tid, tid + 256, ...; a wave reduces in registers, the four waves meet in one RowReduceLds (declared once per kernel,
// __shared__) and are folded in wave order 0..3.  Every rr_block_* helper must be reached by all 256 threads, and ends with a
// barrier: the struct is free for the next helper when one returns (rr_block_lse: see there).
#pragma once
#include "common.h"

struct RowReduceLds {
    float val[4];
    int idx[4];
    float sum[4];
};

// (value, index) maximum, ties to the lower index.  A NaN is never chosen (both comparisons are false).
__device__ __forceinline__ void rr_take_better(float& best, int& bidx, float v, int i) {
    if (v > best || (v == best && i < bidx)) {
        best = v;
        bidx = i;
    }
}

// over the entries a thread owns (row in LDS or in global memory); no entry chosen: value -inf, index 0x7fffffff
__device__ __forceinline__ void rr_local_best(const float* row, int V, int tid, float& best, int& bidx) {
    best = -INFINITY;
    bidx = 0x7fffffff;
    for (int i = tid; i < V; i += 256) rr_take_better(best, bidx, row[i], i);
}

// over the workgroup's per-thread pairs: every thread returns the winner
__device__ __forceinline__ void rr_block_argmax(RowReduceLds& s, int tid, float& best, int& bidx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        rr_take_better(best, bidx, ov, oi);
    }
    if ((tid & 63) == 0) {
        s.val[tid >> 6] = best;
        s.idx[tid >> 6] = bidx;
    }
    __syncthreads();
    best = s.val[0];
    bidx = s.idx[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) rr_take_better(best, bidx, s.val[w], s.idx[w]);
    __syncthreads();
}

// maximum of the per-thread maxima v
__device__ __forceinline__ float rr_block_max(RowReduceLds& s, int tid, float v) {
    v = wave_max(v);
    if ((tid & 63) == 0) s.val[tid >> 6] = v;
    __syncthreads();
    const float m = fmaxf(fmaxf(s.val[0], s.val[1]), fmaxf(s.val[2], s.val[3]));
    __syncthreads();
    return m;
}

// log(sum_i exp(row[i] - rmax)): per thread in ascending i, per wave, then (s0 + s1) + (s2 + s3).  The sums have slots of their
// own, which no other helper touches, and this helper alone ends without a barrier (a second one behind the read measured 4 us
// on a 48 us logsoftmax_topk launch): the slots are free again once every thread has passed any later barrier, so between two
// calls of rr_block_lse there must be another rr_block_* helper - in every kernel the next row's maximum.
__device__ __forceinline__ float rr_block_lse(RowReduceLds& s, const float* row, int V, int tid, float rmax) {
    float sum = 0.f;
    for (int i = tid; i < V; i += 256) sum += expf(row[i] - rmax);
    sum = wave_sum(sum);
    if ((tid & 63) == 0) s.sum[tid >> 6] = sum;
    __syncthreads();
    return logf((s.sum[0] + s.sum[1]) + (s.sum[2] + s.sum[3]));
}

// k selection rounds on a row in LDS, descending, ties to the lower index: thread 0 hands round r's winner to store(r, index,
// value); the thread that owns it overwrites it with `retire` and rescans its own entries (the others keep their cached best).
// A thread only reads the entries it owns, so a row that every thread staged for itself needs no barrier in front.  A round
// without a winner (NaNs only) reports index 0x7fffffff and value -inf: what to store for it is the caller's decision.
template <typename Store>
__device__ __forceinline__ void rr_select_rounds(RowReduceLds& s, float* row, int V, int tid, int k, float retire, Store store) {
    float mybest;
    int myidx;
    rr_local_best(row, V, tid, mybest, myidx);
    for (int r = 0; r < k; ++r) {
        float best = mybest;
        int bidx = myidx;
        rr_block_argmax(s, tid, best, bidx);
        if (tid == 0) store(r, bidx, best);
        if (r + 1 < k && bidx < V && (bidx & 255) == tid) {  // (behind the last round nothing reads the row again)
            row[bidx] = retire;
            rr_local_best(row, V, tid, mybest, myidx);
        }
    }
}
