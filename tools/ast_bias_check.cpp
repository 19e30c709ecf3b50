// Stand-alone host check of the AST beam search's phrase biasing: the step functions the library's kernels and host twins are built
// from (csrc/ast_bias_search.h over csrc/ctc_bias_search.h) run on the CPU, on automata made in memory, every table and every token
// row a heap block of exactly its size.  The tables are built here (trie, failure links, hits, hashed edges - a small hash_bits among
// them, so that probe runs wrap).  Checked against a naive rescan of the token list that knows no automaton:
//   * ab_fold's node is the longest suffix of the labels since the last restart that begins a phrase, and ab_step from the node before
//     gives the same node as folding the whole row (what cn_decode_ast carries is what recomputation gives);
//   * ab_term of every candidate - the vocabulary, eos, ids below and above it - is the rescan's float32 term, bit for bit, and
//     ab_term_chain over ab_chain's nodes (the top-k kernel's form) gives the same bits;
//   * the terms along a row plus the eos term sum to the rescan's banked score (the scores are dyadic: exactly);
//   * nodes outside the table count as the root, and a descriptor with the root alone reads no table (its pointers are null).
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/ast_bias_check.cpp -o ast_bias_check
// Exit status 0 when every check held.
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>

#include "ast_bias_search.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);             \
                fprintf(stderr, "\n");                    \
            }                                             \
        }                                                 \
    } while (0)

namespace {

typedef std::vector<int> Labels;
typedef std::map<Labels, float> Phrases;  // phrase -> per-piece score

// float32(len) * float32(the largest score of the phrases that begin with `prefix`); false when none does
bool prefix_value(const Phrases& ph, const int* prefix, int n, float* value) {
    bool any = false;
    float best = 0.f;
    for (const auto& p : ph)
        if ((int)p.first.size() >= n && std::equal(prefix, prefix + n, p.first.begin())) {
            best = any ? std::max(best, p.second) : p.second;
            any = true;
        }
    *value = (float)n * best;
    return any;
}

// The naive scan of a token row: `seg` the labels since the last restart (negative ids skipped), `banked` what completed phrases gave
struct Scan {
    Labels seg;
    double banked = 0.0;
};
bool completes(const Phrases& ph, const Labels& seg, float* v) {  // the longest suffix of seg that is a listed phrase
    for (size_t k = 0; k < seg.size(); ++k)
        if (ph.count(Labels(seg.begin() + k, seg.end()))) {
            prefix_value(ph, seg.data() + k, (int)(seg.size() - k), v);
            return true;
        }
    return false;
}
Labels open_match(const Phrases& ph, const Labels& seg, float* v) {  // the longest suffix of seg that begins a phrase
    *v = 0.f;
    if (ph.empty()) return Labels();
    for (size_t k = 0; k < seg.size(); ++k)
        if (prefix_value(ph, seg.data() + k, (int)(seg.size() - k), v)) return Labels(seg.begin() + k, seg.end());
    *v = 0.f;
    return Labels();
}
Scan scan(const Phrases& ph, const int* tok, int n) {
    Scan s;
    for (int i = 0; i < n; ++i) {
        if (tok[i] < 0) continue;
        s.seg.push_back(tok[i]);
        float v;
        if (completes(ph, s.seg, &v)) s.banked += (double)v, s.seg.clear();
    }
    return s;
}
float naive_term(const Phrases& ph, const Scan& s, int eos, int V, int c) {
    if (ph.empty()) return 0.f;
    float vn, v2, gain = 0.f;
    const Labels n = open_match(ph, s.seg, &vn);
    if (c == eos) return n.empty() ? 0.f : -vn;
    if (c < 0 || c >= V) return 0.f;
    Labels seg = s.seg;
    seg.push_back(c);
    if (completes(ph, seg, &gain))
        v2 = 0.f;
    else
        open_match(ph, seg, &v2);
    return (float)(((double)gain + (double)v2) - (double)vn);
}

struct Automaton {
    std::unique_ptr<int64_t[]> keys;
    std::unique_ptr<int32_t[]> child, fail;
    std::unique_ptr<float[]> value, bank;
    std::unique_ptr<uint8_t[]> reset;
    std::map<Labels, int> node;
    cn_bias_desc d;
};

std::unique_ptr<Automaton> build(const Phrases& ph, int hash_bits) {
    std::unique_ptr<Automaton> a(new Automaton);
    std::vector<std::map<int, int>> kids(1);
    std::vector<Labels> label(1);
    for (const auto& p : ph) {
        int n = 0;
        for (int c : p.first) {
            if (!kids[n].count(c)) {
                kids[n][c] = (int)kids.size();
                kids.emplace_back();
                Labels l = label[n];
                l.push_back(c);
                label.push_back(l);
            }
            n = kids[n][c];
        }
    }
    const int N = (int)kids.size();
    for (int n = 0; n < N; ++n) a->node[label[n]] = n;
    a->fail.reset(new int32_t[N]()), a->value.reset(new float[N]()), a->bank.reset(new float[N]()), a->reset.reset(new uint8_t[N]());
    for (int n = 1; n < N; ++n) {
        const Labels& l = label[n];
        prefix_value(ph, l.data(), (int)l.size(), &a->value[n]);
        for (size_t k = 1; k <= l.size(); ++k)  // the longest proper suffix that is a node
            if (a->node.count(Labels(l.begin() + k, l.end()))) {
                a->fail[n] = a->node[Labels(l.begin() + k, l.end())];
                break;
            }
        for (size_t k = 0; k < l.size(); ++k)  // the longest suffix, the node included, that is a phrase
            if (ph.count(Labels(l.begin() + k, l.end()))) {
                a->reset[n] = 1;
                prefix_value(ph, l.data() + k, (int)(l.size() - k), &a->bank[n]);
                break;
            }
    }
    int slots = 2;
    while (slots < 2 * N) slots *= 2;
    a->keys.reset(new int64_t[slots]), a->child.reset(new int32_t[slots]());
    std::fill(a->keys.get(), a->keys.get() + slots, (int64_t)-1);
    const uint32_t mask = (uint32_t)slots - 1u, hmask = hash_bits >= 32 ? 0xffffffffu : (1u << hash_bits) - 1u;
    for (int n = 0; n < N; ++n)
        for (const auto& e : kids[n]) {
            uint32_t at = cb_hash(n, e.first) & hmask & mask;
            while (a->keys[at] >= 0) at = (at - 1u) & mask;
            a->keys[at] = (int64_t)(((uint64_t)n << 32) | (uint32_t)e.first);
            a->child[at] = e.second;
        }
    a->d = cn_bias_desc{a->keys.get(), a->child.get(), a->fail.get(), a->value.get(), a->bank.get(), a->reset.get(), slots, N, hash_bits, 0};
    return a;
}

uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

void check_set(const char* name, const Phrases& ph, int hash_bits, int V, int eos, std::mt19937& rng) {
    const std::unique_ptr<Automaton> a = build(ph, hash_bits);
    const cn_bias_desc& d = a->d;
    CHECK(cb_check_desc(d).empty(), "%s: the descriptor is refused", name);
    Labels used;
    for (const auto& p : ph)
        for (int c : p.first) used.push_back(c);
    used.push_back(V - 1);
    std::vector<Labels> rows;
    rows.push_back(Labels());
    for (const auto& p : ph) {  // each phrase whole, cut short, and behind another one
        rows.push_back(p.first);
        rows.push_back(Labels(p.first.begin(), p.first.end() - 1));
        Labels glued = ph.begin()->first;
        glued.insert(glued.end(), p.first.begin(), p.first.end());
        rows.push_back(glued);
    }
    for (int r = 0; r < 60; ++r) {
        Labels row(rng() % 41);
        for (int& t : row) t = rng() % 16 == 0 ? (rng() % 2 ? -1 - (int)(rng() % 3) : V + (int)(rng() % 5)) : used[rng() % used.size()];
        rows.push_back(row);
    }
    for (const Labels& row : rows) {
        const int n = (int)row.size();
        std::unique_ptr<int32_t[]> tok(new int32_t[n]);  // (exactly the row: a read past it is a heap overflow)
        std::copy(row.begin(), row.end(), tok.get());
        double total = 0.0;
        int carried = 0;
        for (int i = 0; i <= n; ++i) {
            const Scan s = scan(ph, tok.get(), i);
            float vopen;
            const Labels open = open_match(ph, s.seg, &vopen);
            const int node = ab_fold(d, tok.get(), i);
            CHECK(a->node.count(open) && node == a->node[open], "%s: node %d of a row of %d tokens", name, node, i);
            CHECK(node == carried, "%s: the carried node %d is not the recomputed %d", name, carried, node);
            int32_t chain[AB_CHAIN];
            const int m = d.nodes > 1 ? ab_chain(d, node, chain) : 0;
            CHECK(m <= AB_CHAIN && (m == 0 || chain[m - 1] == 0 || m == AB_CHAIN), "%s: a chain of %d nodes", name, m);
            const float vn = d.nodes > 1 && node != 0 ? d.value[node] : 0.f;
            for (int c = -2; c < V + 3; ++c) {
                const float want = naive_term(ph, s, eos, V, c), got = ab_term(d, node, eos, V, c);
                CHECK(bits(want) == bits(got), "%s: term of %d behind %d tokens: %g, the rescan gives %g", name, c, i, got, want);
                if (m > 0) CHECK(bits(ab_term_chain(d, chain, m, vn, eos, V, c)) == bits(got), "%s: the chain form differs at %d", name, c);
            }
            if (i < n) {
                total += (double)ab_term(d, node, eos, 0x7fffffff, tok[i]);
                carried = ab_step(d, carried, tok[i]);
            } else {
                total += (double)ab_term(d, node, eos, 0x7fffffff, eos);
                // (an id above V has a term when the ids are not bounded - it breaks the match - so the sum holds for every row)
                CHECK(total == s.banked, "%s: the terms sum to %.17g, the banked score is %.17g", name, total, s.banked);
            }
        }
    }
    // nodes outside the table are the root
    for (int c = 0; c < V; ++c) {
        CHECK(bits(ab_term(d, d.nodes, eos, V, c)) == bits(ab_term(d, 0, eos, V, c)), "%s: node `nodes` is not the root", name);
        CHECK(bits(ab_term(d, -5, eos, V, c)) == bits(ab_term(d, 0, eos, V, c)), "%s: node -5 is not the root", name);
        CHECK(ab_step(d, d.nodes + 7, c) == ab_step(d, 0, c), "%s: ab_step from a node outside the table", name);
    }
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    const int V = 12, eos = 2;
    Labels longp;
    for (int i = 0; i < 32; ++i) longp.push_back(3 + (i % 8 == 7 ? 1 : i % 3) + (i % 8 == 3 ? 4 : 0));
    const Phrases sets[] = {
        {},
        {{{3}, 2.f}},
        {{{3, 4, 5}, 2.f}, {{3, 6}, 3.f}, {{3, 4, 7}, 0.5f}, {{5, 8, 4}, 2.f}},
        {{{3, 4, 5, 6}, 2.f}, {{4, 5}, 3.f}, {{5, 8, 4}, 0.5f}},
        {{{5, 8}, 2.f}, {{5, 8, 4}, 3.f}, {{3, 6}, 0.5f}},
        {{{3, 4, 4, 5}, 2.f}, {{4, 5, 5}, 3.f}, {{5, 5}, 0.5f}},
        {{longp, 0.5f}, {{5, 8, 4}, 2.f}},
        {{{3, 6}, -1.f}, {{5, 8, 4}, -1.f}, {{9, 5}, 2.f}},
        {{{3, 4, 5, 6, 7}, 2.f}, {{4, 5, 6, 10}, 0.5f}, {{5, 6, 9}, 3.f}, {{6, 8, 3}, 2.f}, {{3, 8}, 0.5f}},  // a chain of three links
    };
    const char* names[] = {"none", "one_piece", "shared_prefix", "interior", "extends", "doubled", "long", "negative", "chain"};
    for (size_t i = 0; i < sizeof(sets) / sizeof(sets[0]); ++i)
        for (int hash_bits : {32, 1, 0}) check_set(names[i], sets[i], hash_bits, V, eos, rng);
    // the root alone reads no table
    cn_bias_desc empty{};
    empty.slots = 1, empty.nodes = 1;
    const int32_t row[3] = {3, 4, 5};
    CHECK(cb_check_desc(empty).empty() && ab_fold(empty, row, 3) == 0 && ab_step(empty, 5, 3) == 0, "the root alone");
    for (int c = -1; c <= V; ++c) CHECK(bits(ab_term(empty, 0, eos, V, c)) == 0u, "the root alone: term of %d", c);
    empty.nodes = 0;
    CHECK(cb_check_desc(empty).empty() && ab_fold(empty, row, 3) == 0 && bits(ab_term(empty, 3, eos, V, 3)) == 0u, "no node at all");
    if (failures) {
        fprintf(stderr, "ast_bias_check: %d check(s) failed\n", failures);
        return 1;
    }
    printf("ast_bias_check: all checks held\n");
    return 0;
}
