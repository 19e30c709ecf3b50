// Weighted edit alignment of id sequences: the step functions the kernel (edit_align.hip) and the serial host entry
// (cn_edit_align_host; tools/edit_align_check.cpp builds it with a plain C++ compiler under sanitizers) are both made of.  The
// contract is in include/cassnat_hip_score.h.
//
// A row of the table is a prefix minimum: with t[j] = min(diagonal, up), D[i][j] = c_ins * j + min_{k <= j}(t[k] - c_ins * k).  Both
// sides walk a row in chunks of 64 hyp positions (on the device a wave scan each) and carry the minimum from chunk to chunk.  The
// move into a cell is found from the finished D[i][j] in the tie order (diagonal, up, left), so the scan order cannot change it.
// The moves are 2 bits per cell, stored as two 64-bit masks per (row, chunk of 64 columns): bit j % 64 of word 0 / 1 is bit 0 / 1 of
// the move into (i, j) - on the device one __ballot each.  Rows 1 .. R are stored (row i at index i - 1); row 0 and column 0 are
// known without a table.  A move: 0 diagonal on equal ids, 3 diagonal on different ids, 1 up (deletion), 2 left (insertion).
#pragma once
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cassnat_hip_score.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define EA_HD __host__ __device__ __forceinline__
#else
#define EA_HD inline
#endif

constexpr int EA_THREADS = 64;                // one wave per pair
constexpr int EA_MAX_N = 1 << 20, EA_MAX_LEN = 8192, EA_MAX_COST = 255;
constexpr size_t EA_LDS_CAP = 160 * 1024;     // the dynamic LDS this kernel requests: all of a gfx950 compute unit's
constexpr int EA_MOVE_C = 0, EA_MOVE_D = 1, EA_MOVE_I = 2, EA_MOVE_S = 3;

struct EditArgs {
    const int32_t* ref = nullptr;
    const int64_t* ref_begin = nullptr;  // [N]
    const int32_t* ref_len = nullptr;    // [N]
    const int32_t* hyp = nullptr;
    const int64_t* hyp_begin = nullptr;  // [N]
    const int32_t* hyp_len = nullptr;    // [N]
    const int64_t* ops_begin = nullptr;  // [N]
    int64_t ref_total = 0, hyp_total = 0, ops_total = 0;
    int32_t N = 0, max_ref = 0, max_hyp = 0, c_sub = 1, c_ins = 1, c_del = 1;
    int32_t* cost = nullptr;      // [N]
    int32_t* counts = nullptr;    // [N][4]
    int32_t* path_len = nullptr;  // [N]
    uint8_t* ops = nullptr;
    unsigned long long* bp = nullptr;  // device scratch of ea_scratch_bytes (the scratch form only)
};

EA_HD int ea_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
EA_HD int ea_chunks(int cols) { return (cols + 63) >> 6; }

// do the three spans of a pair of R x H stay inside their buffers?
EA_HD bool ea_span_ok(const EditArgs& a, int64_t rb, int64_t hb, int64_t ob, int R, int H) {
    return rb >= 0 && hb >= 0 && ob >= 0 && rb <= a.ref_total - R && hb <= a.hyp_total - H && ob <= a.ops_total - R - H;
}

// the two candidates of cell (i, j >= 1) that do not depend on the row itself
EA_HD void ea_cand(int prev_jm1, int prev_j, bool eq, int c_sub, int c_del, int* diag, int* up) {
    *diag = prev_jm1 + (eq ? 0 : c_sub);
    *up = prev_j + c_del;
}

// the move into a cell whose finished value is d: the first of (diagonal, up, left) that attains it; column 0 points up
EA_HD int ea_move(int d, int diag, int up, bool eq, bool col0) {
    if (col0) return EA_MOVE_D;
    if (d == diag) return eq ? EA_MOVE_C : EA_MOVE_S;
    return d == up ? EA_MOVE_D : EA_MOVE_I;
}

EA_HD int ea_bp_move(unsigned long long lo, unsigned long long hi, int j) { return (int)((lo >> (j & 63)) & 1ull) | ((int)((hi >> (j & 63)) & 1ull) << 1); }

// the output code of a move: 0 = C, 1 = S, 2 = D, 3 = I
EA_HD int ea_op(int move) { return move == EA_MOVE_C ? 0 : (move == EA_MOVE_S ? 1 : move + 1); }

// The walk from (R, H) to (0, 0) over bp [R][chunks][2]: the codes go to back[0 .. P) in backward order, counts[4] (C, S, D, I) are
// added up; returns P.  A counted loop: whatever the table holds, it ends after R + H steps and never leaves the table.
EA_HD int ea_walk(const unsigned long long* bp, int chunks, int R, int H, uint8_t* back, int* counts) {
    int i = R, j = H, P = 0;
    for (int step = 0; step < R + H; ++step) {
        if (i == 0 && j == 0) break;
        int mv;
        if (i == 0)
            mv = EA_MOVE_I;
        else if (j == 0)
            mv = EA_MOVE_D;
        else {
            const unsigned long long* w = bp + ((size_t)(i - 1) * chunks + (j >> 6)) * 2;
            mv = ea_bp_move(w[0], w[1], j);
        }
        const int op = ea_op(mv);
        back[P++] = (uint8_t)op;
        ++counts[op];
        if (mv != EA_MOVE_I) --i;
        if (mv != EA_MOVE_D) --j;
    }
    return P;
}

// ---- launch geometry (host) ------------------------------------------------------------------------------------------------------
// bytes of dynamic LDS in front of the back-pointers: two rows and the hyp ids (max_hyp + 1 int32 each), the backward path
inline size_t ea_row_words(int max_hyp) { return ((size_t)max_hyp + 1 + 3) & ~(size_t)3; }
inline size_t ea_lds_fixed(int max_ref, int max_hyp) { return (3 * ea_row_words(max_hyp) * 4 + (size_t)max_ref + (size_t)max_hyp + 15) & ~(size_t)15; }
inline size_t ea_bp_bytes(int max_ref, int max_hyp) { return (size_t)max_ref * ea_chunks(max_hyp + 1) * 16; }
inline bool ea_bp_in_lds(int max_ref, int max_hyp, long long limit) {
    return ea_lds_fixed(max_ref, max_hyp) + ea_bp_bytes(max_ref, max_hyp) <= EA_LDS_CAP &&
           (limit < 0 || ((long long)max_ref + 1) * ((long long)max_hyp + 1) <= limit);
}
// device scratch the launch needs in a.bp (0: the back-pointers live in LDS, or there are none)
inline size_t ea_scratch_bytes(int N, int max_ref, int max_hyp, long long limit) {
    return ea_bp_in_lds(max_ref, max_hyp, limit) ? 0 : (size_t)N * ea_bp_bytes(max_ref, max_hyp);
}
static_assert(3 * (((size_t)EA_MAX_LEN + 4) & ~(size_t)3) * 4 + 2 * (size_t)EA_MAX_LEN + 16 <= EA_LDS_CAP, "the longest pair must fit the LDS in the scratch form");

// what is refused before anything runs (empty: fine)
inline std::string ea_check(const EditArgs& a) {
    if (!a.ref || !a.ref_begin || !a.ref_len || !a.hyp || !a.hyp_begin || !a.hyp_len || !a.ops_begin || !a.cost || !a.counts || !a.path_len || !a.ops)
        return "null argument";
    if (a.N < 1 || a.N > EA_MAX_N) return "N must lie in 1 .. " + std::to_string(EA_MAX_N);
    if (a.max_ref < 0 || a.max_ref > EA_MAX_LEN) return "max_ref must lie in 0 .. " + std::to_string(EA_MAX_LEN);
    if (a.max_hyp < 0 || a.max_hyp > EA_MAX_LEN) return "max_hyp must lie in 0 .. " + std::to_string(EA_MAX_LEN);
    for (const int32_t c : {a.c_sub, a.c_ins, a.c_del})
        if (c < 1 || c > EA_MAX_COST) return "the costs must lie in 1 .. " + std::to_string(EA_MAX_COST);
    if (a.ref_total < 0 || a.hyp_total < 0 || a.ops_total < 0) return "the buffer sizes must not be negative";
    return "";
}

// ---- the serial twin: one pair, every pointer a host pointer ---------------------------------------------------------------------
inline void ea_align_host(const EditArgs& a, int n) {
    const int R = ea_clamp(a.ref_len[n], 0, a.max_ref), H = ea_clamp(a.hyp_len[n], 0, a.max_hyp), chunks = ea_chunks(H + 1);
    const int64_t rb = a.ref_begin[n], hb = a.hyp_begin[n], ob = a.ops_begin[n];
    int32_t* counts = a.counts + (size_t)n * 4;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    a.path_len[n] = 0;
    if (!ea_span_ok(a, rb, hb, ob, R, H)) {
        a.cost[n] = -1;
        return;
    }
    const int32_t* ref = a.ref + rb;
    const int32_t* hyp = a.hyp + hb;
    std::vector<int> prev((size_t)H + 1), cur((size_t)H + 1);
    std::vector<unsigned long long> bp((size_t)R * chunks * 2, 0ull);
    for (int j = 0; j <= H; ++j) prev[j] = j * a.c_ins;
    for (int i = 1; i <= R; ++i) {
        int carry = INT_MAX;
        for (int base = 0; base <= H; base += 64) {  // (a chunk: what one wave scans)
            for (int j = base; j <= H && j < base + 64; ++j) {
                int diag = 0, up = 0;
                const bool eq = j > 0 && ref[i - 1] == hyp[j - 1];
                if (j > 0) ea_cand(prev[j - 1], prev[j], eq, a.c_sub, a.c_del, &diag, &up);
                const int t = j > 0 ? (diag < up ? diag : up) : i * a.c_del;
                const int v = t - a.c_ins * j;
                if (v < carry) carry = v;
                const int d = carry + a.c_ins * j;
                cur[j] = d;
                const int mv = ea_move(d, diag, up, eq, j == 0);
                unsigned long long* w = bp.data() + ((size_t)(i - 1) * chunks + (j >> 6)) * 2;
                w[0] |= (unsigned long long)(mv & 1) << (j & 63);
                w[1] |= (unsigned long long)(mv >> 1) << (j & 63);
            }
        }
        prev.swap(cur);
    }
    a.cost[n] = prev[H];
    std::vector<uint8_t> back((size_t)R + H + 1);
    int c4[4] = {0, 0, 0, 0};
    const int P = ea_walk(bp.data(), chunks, R, H, back.data(), c4);
    for (int k = 0; k < P; ++k) a.ops[ob + k] = back[P - 1 - k];
    for (int k = 0; k < 4; ++k) counts[k] = c4[k];
    a.path_len[n] = P;
}

// check, then every pair in turn; the message of a refusal goes to *err
inline int ea_run_host(const EditArgs& a, std::string* err) {
    const std::string bad = ea_check(a);
    if (!bad.empty()) {
        *err = bad;
        return -1;
    }
    for (int32_t n = 0; n < a.N; ++n) ea_align_host(a, n);
    return 0;
}

#ifdef __HIPCC__
// one launch; a.bp must hold ea_scratch_bytes(N, max_ref, max_hyp, bp_lds_limit) bytes when that is not 0           (edit_align.hip)
int launch_edit_align(const EditArgs& a, long long bp_lds_limit, hipStream_t s);
#endif
