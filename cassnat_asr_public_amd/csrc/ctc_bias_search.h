// CTC prefix beam search with contextual phrase biasing: score_lm of the shared search (ctc_search.h) formed from a phrase automaton -
// the edge lookup, the step of a hypothesis' (node, banked) state and a candidate's score_lm - and the serial host search
// (cn_ctc_bias_beam_host; tools/ctc_bias_check.cpp builds it with a plain C++ compiler under sanitizers).  The kernel (ctc_beam.hip)
// and the host search are made of the same functions.
//
// The contract is in include/cassnat_hip_ctc_bias.h.  Unlike the n-gram variant, whose look-ups are per kept hypothesis, what a label
// adds here depends on the parent's node AND on the label: every candidate walks the hashed edges itself (cb_step), and a winner
// takes over the state its candidate found.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cassnat_hip_ctc_bias.h"
#include "ctc_search.h"

constexpr int CB_MAX_PHRASE = 32;  // pieces of the longest phrase = the longest failure chain

struct CtcBiasArgs : CtcBeamArgs {  // (out.score_lm is written)
    cn_bias_desc d;
};
inline CtcBiasArgs ctc_bias_args(const cn_bias_desc& d, const CtcBeamArgs& search) {
    CtcBiasArgs a;
    static_cast<CtcBeamArgs&>(a) = search;
    a.d = d;
    return a;
}
#ifdef __HIPCC__
int launch_ctc_bias_beam(const CtcBiasArgs& a, hipStream_t s);
#endif

struct CbState {  // 16 bytes
    int32_t node, pad;
    double banked;
};

NG_HD CbState cb_init() {
    CbState s;
    s.node = 0, s.pad = 0, s.banked = 0.0;
    return s;
}

// where the probing of (node, piece) starts, before the masks
NG_HD uint32_t cb_hash(int node, int piece) {
    uint32_t h = (uint32_t)node * 0x9E3779B1u ^ (uint32_t)piece * 0x85EBCA6Bu;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

// the child of `node` under label c, or -1 (a child outside the node table counts as none); at most d.slots probes
NG_HD int cb_edge(const cn_bias_desc& d, int node, int c) {
    const int64_t key = (int64_t)(((uint64_t)(uint32_t)node << 32) | (uint32_t)c);
    const uint32_t mask = (uint32_t)d.slots - 1u;
    uint32_t at = cb_hash(node, c) & (d.hash_bits >= 32 ? 0xffffffffu : (1u << d.hash_bits) - 1u) & mask;
    for (int i = 0; i < d.slots; ++i) {
        const int64_t k = d.edge_keys[at];
        if (k == key) {
            const int child = d.edge_child[at];
            return (uint32_t)child < (uint32_t)d.nodes ? child : -1;
        }
        if (k < 0) return -1;
        at = (at - 1u) & mask;  // (downwards: a small hash_bits makes runs that wrap past slot 0)
    }
    return -1;
}

// the state of `s` with label c appended (c < 0: stay)
NG_HD CbState cb_step(const cn_bias_desc& d, CbState s, int c) {
    if (c < 0 || d.nodes <= 1) return s;
    int n = s.node, child = cb_edge(d, n, c);
    for (int i = 0; i < CB_MAX_PHRASE && child < 0 && n != 0; ++i) {
        n = d.fail[n];
        if ((uint32_t)n >= (uint32_t)d.nodes) n = 0;
        child = cb_edge(d, n, c);
    }
    n = child >= 0 ? child : 0;
    if (n != 0 && d.reset[n]) {  // (the root ends no phrase: most candidates miss, and stop after the one probe)
        s.banked += (double)d.bank[n];
        n = 0;
    }
    s.node = n;
    return s;
}

// score_lm of a hypothesis, or of a candidate, in state s (value[0] is 0: not read)
NG_HD double cb_slm(const cn_bias_desc& d, const CbState& s) { return s.node != 0 ? s.banked + (double)d.value[s.node] : s.banked; }

// ---- host only -------------------------------------------------------------------------------------------------------------------
inline std::string cb_check_desc(const cn_bias_desc& d) {
    if (d.slots < 1 || (d.slots & (d.slots - 1))) return "the slot count of the bias table must be a power of two";
    if (d.nodes < 0) return "the node count of the bias automaton must not be negative";
    if (d.hash_bits < 0 || d.hash_bits > 32) return "hash_bits of the bias table must lie in 0 .. 32";
    if (d.nodes > 1 && (!d.edge_keys || !d.edge_child || !d.fail || !d.value || !d.bank || !d.reset)) return "null table in the bias descriptor";
    return "";
}

// "" when the arguments can be searched (pointers of the caller's side: not dereferenced here), else what is wrong
inline std::string cb_check(const CtcBiasArgs& a, bool need_scratch) {
    const CtcBeamOut& o = a.out;
    if (!a.logp || !a.size_ratio || (a.P > 0 && !a.top_idx) || !o.hyp || !o.hyp_len || !o.score || !o.score_lm || !o.p_blk || !o.p_nblk ||
        !o.n_out || (need_scratch && (!a.hist_parent || !a.hist_tok)))
        return "null argument";
    if (const char* bad = cs_check_limits(a.W, a.P, 0, 0)) return bad;
    const std::string bad = cb_check_desc(a.d);
    if (!bad.empty()) return bad;
    if (a.B < 1 || a.Tp < 1 || a.V < 1) return "B, T' and V must be positive";
    if (a.blank < 0 || a.blank >= a.V) return "blank must be an id of the vocabulary";
    if (const char* cap = cs_check_limits(a.W, a.P, a.Tp, o.Lmax)) return cap;
    if (!(a.lp == a.lp)) return "length_penalty must be a number";
    return "";
}

// utterance b of `a`, every pointer a host pointer; the back-pointers are kept here, a.hist_parent / a.hist_tok are not used.  The
// order comes from std::stable_sort: the independent check of cs_rank.
inline void cb_search_host(const CtcBiasArgs& a, int b) {
    struct Cand {
        CsCand c;
        CbState st;
        double key;
    };
    const cn_bias_desc& d = a.d;
    const int W = a.W, P = a.P;
    std::vector<CsKept> kept(W);
    std::vector<int> blast(W), order;
    std::vector<CbState> st[2] = {std::vector<CbState>(W), std::vector<CbState>(W)};
    std::vector<Cand> cand;
    std::vector<unsigned char> hpar((size_t)a.Tp * W);
    std::vector<int> htok((size_t)a.Tp * W);
    const float* logp = a.logp + (long long)b * a.Tp * a.V;
    const int* top = a.top_idx + (long long)b * a.Tp * P;
    const int ssz = cs_src_size(a.size_ratio[b], a.Tp);
    kept[0] = CsKept{0.0, 0.0, 0.0, CS_LOGZERO, 0};  // score_ctc 0, p_blk logone, p_nblk logzero, hyp []
    blast[0] = -1;
    st[0][0] = cb_init();
    int nb = 1, steps = 0, cur = 0;
    for (int t = 0; t <= ssz && t < a.Tp; ++t) {
        const float* row = logp + (long long)t * a.V;
        if (cs_skip_frame(row[a.blank])) continue;
        cand.clear();
        order.clear();
        for (int k = 0; k < nb; ++k)
            for (int j = 0; j <= P; ++j) {
                const int c = j == 0 ? -1 : top[(long long)t * P + (j - 1)];
                Cand x;
                x.c = cs_candidate(row, a.V, a.blank, k, j == 0, c, kept[k].p_blk, kept[k].p_nblk, blast[k], kept[k].len);
                if (x.c.par < 0) continue;
                x.st = cb_step(d, st[cur][k], x.c.tok);
                x.key = cs_key(x.c.tot, cb_slm(d, x.st), a.lp, x.c.len);
                order.push_back((int)cand.size());
                cand.push_back(x);
            }
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cand[x].key > cand[y].key; });
        const int keep = (int)order.size() < W ? (int)order.size() : W;
        std::vector<CsKept> next(W);
        for (int r = 0; r < keep; ++r) {
            const CsCand& c = cand[order[r]].c;
            next[r] = CsKept{c.tot, 0.0, c.pb, c.pnb, c.len};
            blast[r] = c.last;  // (every parent's state was read into `cand` above)
            hpar[(size_t)steps * W + r] = (unsigned char)c.par;
            htok[(size_t)steps * W + r] = c.tok;
            st[cur ^ 1][r] = cand[order[r]].st;
        }
        kept.swap(next);
        nb = keep, ++steps, cur ^= 1;
    }
    // the open match is given up; one more stable sort by the same key
    std::vector<double> key(nb);
    order.clear();
    for (int r = 0; r < nb; ++r) {
        kept[r].score_lm = st[cur][r].banked;
        key[r] = cs_key(kept[r].score, kept[r].score_lm, a.lp, kept[r].len);
        order.push_back(r);
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] > key[y]; });
    a.out.n_out[b] = nb;
    for (int r = 0; r < W; ++r)
        cs_write_row(a.out, (long long)b * W + r, hpar.data(), htok.data(), 0, W, steps, r < nb ? order[r] : -1, kept[r < nb ? order[r] : 0]);
}
