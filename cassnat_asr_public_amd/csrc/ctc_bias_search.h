// CTC prefix beam search with contextual phrase biasing: score_lm of the shared search (ctc_search.h) formed from a phrase automaton -
// the edge lookup, the step of a hypothesis' (node, banked) state and a candidate's score_lm.  The kernel (ctc_beam.hip) and the
// serial host search (ctc_search_host.h; cn_ctc_bias_beam_host; tools/ctc_bias_check.cpp builds it with a plain C++ compiler under
// sanitizers) are made of the same functions.
//
// The contract is in include/cassnat_hip_ctc_bias.h.  Unlike the n-gram variant, whose look-ups are per kept hypothesis, what a label
// adds here depends on the parent's node AND on the label: every candidate walks the hashed edges itself (cb_step), and a winner
// takes over the state its candidate found.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/cassnat_hip_ctc_bias.h"
#include "ctc_search.h"

constexpr int CB_MAX_PHRASE = 32;  // pieces of the longest phrase = the longest failure chain

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
