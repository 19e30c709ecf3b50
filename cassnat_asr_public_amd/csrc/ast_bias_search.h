// AST beam search with contextual phrase biasing: what a hypothesis carries (the node of the phrase automaton) and what a candidate
// token adds (its term), made of ctc_bias_search.h's edge lookup and step.  The kernels (ast_bias.hip), the host twins
// (cn_ast_bias_nodes_host / cn_ast_bias_terms_host) and tools/ast_bias_check.cpp, which builds this header with a plain C++ compiler
// under sanitizers, are made of the same functions.  The contract is in include/cassnat_hip_ast_bias.h.
#pragma once
#include "../../include/cassnat_hip_ast_bias.h"
#include "ctc_bias_search.h"

constexpr int AB_CHAIN = CB_MAX_PHRASE + 1;  // a node and its at most 32 failure targets: what cb_step's walk can probe

// a node of the caller's: outside the table (or in a table with the root alone) it is the root
NG_HD int ab_node(const cn_bias_desc& d, int n) { return d.nodes > 1 && (uint32_t)n < (uint32_t)d.nodes ? n : 0; }

// the node of a hypothesis at node n with label c appended (c < 0: stay)
NG_HD int ab_step(const cn_bias_desc& d, int n, int c) {
    CbState s = cb_init();
    s.node = ab_node(d, n);
    return cb_step(d, s, c).node;
}

// the node of the hypothesis tok[0 .. len)
NG_HD int ab_fold(const cn_bias_desc& d, const int32_t* tok, int len) {
    CbState s = cb_init();
    if (d.nodes <= 1) return 0;
    for (int i = 0; i < len; ++i) s = cb_step(d, s, tok[i]);
    return s.node;
}

// the nodes cb_step's walk probes from n, in its order: n, fail[n], ... down to the root, at most AB_CHAIN of them; returns how many
NG_HD int ab_chain(const cn_bias_desc& d, int n, int32_t* chain) {
    int m = 0;
    chain[m++] = n;
    for (int i = 0; i < CB_MAX_PHRASE && n != 0; ++i) {
        n = d.fail[n];
        if ((uint32_t)n >= (uint32_t)d.nodes) n = 0;
        chain[m++] = n;
    }
    return m;
}

// what the walk ends in - child ch, or the root - as a term against the value vn of the node it began at
NG_HD float ab_gain(const cn_bias_desc& d, int ch, float vn) {
    float gain = 0.f;
    if (ch != 0 && d.reset[ch]) {
        gain = d.bank[ch];
        ch = 0;
    }
    const float vch = ch != 0 ? d.value[ch] : 0.f;
    return (float)(((double)gain + (double)vch) - (double)vn);
}

// the term of candidate c over a chain of ab_chain (chain[0] the hypothesis' node, vn its value, 0 at the root); V bounds the ids
NG_HD float ab_term_chain(const cn_bias_desc& d, const int32_t* chain, int m, float vn, int eos, int V, int c) {
    if (c == eos) return chain[0] != 0 ? -vn : 0.f;
    if (c < 0 || c >= V) return 0.f;
    int child = -1;
    for (int j = 0; j < m && child < 0; ++j) child = cb_edge(d, chain[j], c);
    return ab_gain(d, child >= 0 ? child : 0, vn);
}

// the term of candidate c for a hypothesis at node n: cb_step's own walk, one failure link at a time
NG_HD float ab_term(const cn_bias_desc& d, int n, int eos, int V, int c) {
    if (d.nodes <= 1) return 0.f;
    n = ab_node(d, n);
    const float vn = n != 0 ? d.value[n] : 0.f;
    if (c == eos) return n != 0 ? -vn : 0.f;
    if (c < 0 || c >= V) return 0.f;
    int child = cb_edge(d, n, c);
    for (int i = 0; i < CB_MAX_PHRASE && child < 0 && n != 0; ++i) {
        n = d.fail[n];
        if ((uint32_t)n >= (uint32_t)d.nodes) n = 0;
        child = cb_edge(d, n, c);
    }
    return ab_gain(d, child >= 0 ? child : 0, vn);
}

// Where a beam slot's node comes from inside cn_decode_ast: node[pos][s] = ab_step(node[pos - 1][anc[s][pos - 1]], tok[s]), the root
// at position 0.  `out` non-null switches a launch to this form (its `node` argument is then not read); `prev` null is position 0.
struct AbCarry {
    const int32_t* prev = nullptr;  // [slots] the nodes of position pos - 1
    const int32_t* anc = nullptr;   // [slots][ld] the slot that computed a position
    const int32_t* tok = nullptr;   // [slots] the token at position pos
    int32_t* out = nullptr;         // [slots] the nodes of position pos
    int ld = 0, col = 0, slots = 0; // col = pos - 1
};

NG_HD int ab_carried(const cn_bias_desc& d, const AbCarry& cs, int row) {
    if (!cs.prev) return 0;
    const int a = cs.anc[(long long)row * cs.ld + cs.col];
    return ab_step(d, (uint32_t)a < (uint32_t)cs.slots ? cs.prev[a] : 0, cs.tok[row]);
}

#ifdef __HIPCC__
int launch_ast_bias_nodes(const cn_bias_desc& d, const int* tok, int ld, const int* len, int n, int* node_out, hipStream_t s);
int launch_ast_bias_terms(const cn_bias_desc& d, const int* node, const AbCarry& cs, int eos, const int* idx, int n, int K, float* term,
                          hipStream_t s);
int launch_logsoftmax_bias_topk(const float* att, int M, int V, int ldl, float temperature, const cn_bias_desc& d, const int* node,
                                const AbCarry& cs, int eos, int k, int* idx, float* val, hipStream_t s);
#endif
