// CTC token time stamps: the step functions the kernel (ctc_times.hip) and the serial host entry (cn_ctc_token_times_host;
// tools/ctc_times_check.cpp builds it with a plain C++ compiler under sanitizers) are both made of.  The contract is in
// include/cassnat_hip_ctc_times.h.
//
// A forced alignment over the blank-augmented labels in float64 with true -inf, the first of (stay, s-1, s-2) winning a tie.  The
// back-pointers are 2 bits per (frame, state), stored as two 64-bit masks per (frame, chunk of 64 states): bit s % 64 of word 0 / 1
// is bit 0 / 1 of the move into state s - on the device one __ballot each of the wave that owns the chunk.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "../../include/cassnat_hip_ctc_times.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define CT_HD __host__ __device__ __forceinline__
#else
#define CT_HD inline
#endif

constexpr int CT_THREADS = 256;
constexpr int CT_MAX_B = 1 << 16, CT_MAX_TP = 1 << 16, CT_MAX_V = 1 << 20, CT_MAX_LD = 1500;
constexpr int CT_EMIS = 2048;                  // floats of the emission block (at least one frame's states)
constexpr int CT_MAX_FB = 32;                  // frames of an emission block at most
constexpr size_t CT_LDS_CAP = 96 * 1024;       // the dynamic LDS the project requests (launch_ctc_viterbi, launch_beam)

struct CtcTimesArgs {
    const float* logp = nullptr;         // [B][Tp][V]
    const int32_t* frames = nullptr;     // [B]
    const int32_t* labels = nullptr;     // [B][ld]
    const int32_t* label_len = nullptr;  // [B]
    int32_t B = 0, Tp = 0, V = 0, ld = 0, blank = 0;
    int32_t* start = nullptr;  // [B][ld]
    int32_t* end = nullptr;    // [B][ld]
    float* conf = nullptr;     // [B][ld]
    double* score = nullptr;   // [B]
    int32_t* status = nullptr;  // [B]
    unsigned long long* bp = nullptr;  // device scratch of ct_scratch_bytes (the scratch form only)
};

CT_HD int ct_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
CT_HD int ct_chunks(int S) { return (S + 63) >> 6; }
CT_HD bool ct_label_ok(int32_t y, int32_t V, int32_t blank) { return y >= 0 && y < V && y != blank; }

// max(a0, a1, a2) with the first of (stay, s-1, s-2) winning a tie; has1 / has2: the move exists
CT_HD double ct_step(double a0, double a1, double a2, bool has1, bool has2, int* move) {
    double mx = a0;
    int ix = 0;
    if (has1 && a1 > mx) {
        mx = a1;
        ix = 1;
    }
    if (has2 && a2 > mx) {
        mx = a2;
        ix = 2;
    }
    *move = ix;
    return mx;
}

// the move into state s from the two masks of its chunk
CT_HD int ct_bp_move(unsigned long long lo, unsigned long long hi, int s) { return (int)((lo >> (s & 63)) & 1ull) | ((int)((hi >> (s & 63)) & 1ull) << 1); }

// the last label's state wins against the trailing blank on a tie
CT_HD int ct_end_state(int L, double a_label, double a_blank) { return L == 0 ? 0 : (a_label >= a_blank ? 2 * L - 1 : 2 * L); }

// The best path backwards from state `cur` at frame n - 1 over bp [n - 1][chunks][2] (row t - 1: the moves into frame t): st / en [L]
// (all -1 on entry) get the first and last + 1 frame spent in each label's state.  States only fall, so a label's span is one run.
CT_HD void ct_walk(const unsigned long long* bp, int chunks, int n, int cur, int32_t* st, int32_t* en) {
    int open = -1;
    for (int t = n - 1; t >= 0; --t) {
        if (cur & 1) {
            const int u = cur >> 1;
            if (u != open) {
                en[u] = t + 1;
                open = u;
            }
            st[u] = t;
        }
        if (t > 0) {
            const unsigned long long* w = bp + ((size_t)(t - 1) * chunks + (cur >> 6)) * 2;
            cur -= ct_bp_move(w[0], w[1], cur);
        }
    }
}

// the largest log-posterior of label y over frames [s0, e0) of one utterance's rows (0 for a label the walk never entered)
CT_HD float ct_conf(const float* logp, int V, int32_t y, int s0, int e0) {
    if (s0 < 0 || e0 <= s0) return 0.f;
    float c = logp[(size_t)s0 * V + y];
    for (int t = s0 + 1; t < e0; ++t) {
        const float v = logp[(size_t)t * V + y];
        if (v > c) c = v;
    }
    return c;
}

// ---- launch geometry (host) ------------------------------------------------------------------------------------------------------
// bytes of dynamic LDS in front of the back-pointers for rows of Smax states: two alpha rows, the emission block, the path
inline int ct_emis_floats(int Smax) { return Smax > CT_EMIS ? (Smax + 3) & ~3 : CT_EMIS; }
inline size_t ct_lds_fixed(int Smax) { return ((size_t)Smax * 16 + (size_t)ct_emis_floats(Smax) * 4 + (size_t)Smax * 4 + 15) & ~(size_t)15; }
inline size_t ct_bp_bytes(int Tp, int Smax) { return (size_t)(Tp > 1 ? Tp - 1 : 0) * ct_chunks(Smax) * 16; }
inline bool ct_bp_in_lds(int Tp, int ld, long long limit) {
    const int Smax = 2 * ld + 1;
    return ct_lds_fixed(Smax) + ct_bp_bytes(Tp, Smax) <= CT_LDS_CAP && (limit < 0 || (long long)Tp * Smax <= limit);
}
// device scratch the launch needs in a.bp (0: the back-pointers live in LDS)
inline size_t ct_scratch_bytes(int B, int Tp, int ld, long long limit) { return ct_bp_in_lds(Tp, ld, limit) ? 0 : (size_t)B * ct_bp_bytes(Tp, 2 * ld + 1); }

// what is refused before anything runs (empty: fine)
inline std::string ct_check(const CtcTimesArgs& a) {
    if (!a.logp || !a.frames || !a.labels || !a.label_len || !a.start || !a.end || !a.conf || !a.score || !a.status) return "null argument";
    if (a.B < 1 || a.B > CT_MAX_B) return "B must lie in 1 .. " + std::to_string(CT_MAX_B);
    if (a.Tp < 1 || a.Tp > CT_MAX_TP) return "the frame count T' must lie in 1 .. " + std::to_string(CT_MAX_TP);
    if (a.V < 1 || a.V > CT_MAX_V) return "V must lie in 1 .. " + std::to_string(CT_MAX_V);
    if (a.ld < 1 || a.ld > CT_MAX_LD) return "the label row width ld must lie in 1 .. " + std::to_string(CT_MAX_LD);
    if (a.blank < 0 || a.blank >= a.V) return "the blank must lie in [0, V)";
    return "";
}
static_assert((size_t)(2 * CT_MAX_LD + 1) * 24 + 16 <= CT_LDS_CAP, "the widest label row must fit the LDS in the scratch form");

// ---- the serial twin: one utterance, every pointer a host pointer ---------------------------------------------------------------
inline void ct_align_host(const CtcTimesArgs& a, int b) {
    const int n = ct_clamp(a.frames[b], 0, a.Tp), L = ct_clamp(a.label_len[b], 0, a.ld), S = 2 * L + 1, chunks = ct_chunks(S);
    const int32_t* lab = a.labels + (size_t)b * a.ld;
    const float* logp = a.logp + (size_t)b * a.Tp * a.V;
    int32_t* start = a.start + (size_t)b * a.ld;
    int32_t* end = a.end + (size_t)b * a.ld;
    float* conf = a.conf + (size_t)b * a.ld;
    const double ninf = -std::numeric_limits<double>::infinity();
    bool bad = false;
    int rep = 0;
    for (int u = 0; u < L; ++u) {
        if (!ct_label_ok(lab[u], a.V, a.blank)) bad = true;
        if (u > 0 && lab[u] == lab[u - 1]) ++rep;
    }
    const int status = bad ? 2 : (L + rep > n ? 1 : 0);
    a.status[b] = status;
    for (int u = 0; u < L; ++u) {
        start[u] = end[u] = -1;
        conf[u] = 0.f;
    }
    if (status != 0) {
        a.score[b] = ninf;
        return;
    }
    if (n == 0) {  // (then L == 0: the empty path)
        a.score[b] = 0.0;
        return;
    }
    std::vector<int32_t> path(S, a.blank);
    for (int u = 0; u < L; ++u) path[2 * u + 1] = lab[u];
    std::vector<double> prev(S, ninf), next(S, ninf);
    std::vector<unsigned long long> bp((size_t)(n - 1) * chunks * 2, 0ull);
    for (int s = 0; s < S && s < 2; ++s) prev[s] = (double)logp[path[s]];
    for (int t = 1; t < n; ++t) {
        for (int s = 0; s < S; ++s) {
            const bool has2 = (s & 1) && s >= 3 && path[s - 2] != path[s];
            int move;
            const double mx = ct_step(prev[s], s >= 1 ? prev[s - 1] : 0.0, has2 ? prev[s - 2] : 0.0, s >= 1, has2, &move);
            next[s] = mx + (double)logp[(size_t)t * a.V + path[s]];
            unsigned long long* w = bp.data() + ((size_t)(t - 1) * chunks + (s >> 6)) * 2;
            w[0] |= (unsigned long long)(move & 1) << (s & 63);
            w[1] |= (unsigned long long)(move >> 1) << (s & 63);
        }
        prev.swap(next);
    }
    const int cur = ct_end_state(L, L ? prev[2 * L - 1] : 0.0, L ? prev[2 * L] : 0.0);
    a.score[b] = prev[cur];
    ct_walk(bp.data(), chunks, n, cur, start, end);
    for (int u = 0; u < L; ++u) conf[u] = ct_conf(logp, a.V, lab[u], start[u], end[u]);
}

#ifdef __HIPCC__
// one launch; a.bp must hold ct_scratch_bytes(B, Tp, ld, bp_lds_limit) bytes when that is not 0           (ctc_times.hip)
int launch_ctc_token_times(const CtcTimesArgs& a, long long bp_lds_limit, hipStream_t s);
#endif
