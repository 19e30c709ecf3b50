// Stand-alone host check of the CTC prefix beam search with phrase biasing: the step functions and the serial search the library and
// its kernel are built from (csrc/ctc_search_host.h over csrc/ctc_search.h and csrc/ctc_bias_search.h) run on the CPU, on automata and random log-posteriors made in
// memory, every array a heap block of exactly the size the search was told.  The automaton's tables are built here (trie, failure
// links, hits, hashed edges - a small hash_bits among them, so that probe runs wrap).  Checked:
//   * ctc_search_host with a bias descriptor gives the bytes of a naive search that keeps every hypothesis' labels and rescans ALL of them against the phrase
//     list for every candidate (no automaton, no state): hypotheses, order, lengths and all four scores;
//   * the beam comes back sorted by its key, lengths and labels are in range;
//   * with the root alone (with and without tables) score_lm is 0 and every other output is the same bytes whatever the descriptor;
//   * a pruned label outside [0, V) makes no candidate;
//   * the refusals refuse.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/ctc_bias_check.cpp -o ctc_bias_check
// Exit status 0 when every check held.
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>

#include "ctc_search_host.h"

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

// score_lm of a label sequence by a direct scan: behind every label the longest suffix of the labels since the last restart that is a
// listed phrase banks its value and restarts; with `open` the value of the longest suffix that begins a phrase is added
double rescan(const Phrases& ph, const Labels& h, bool open) {
    double banked = 0.0;
    size_t from = 0;
    for (size_t i = 0; i < h.size(); ++i)
        for (size_t k = from; k <= i; ++k)
            if (ph.count(Labels(h.begin() + k, h.begin() + i + 1))) {
                float v;
                prefix_value(ph, h.data() + k, (int)(i + 1 - k), &v);
                banked += (double)v;
                from = i + 1;
                break;
            }
    if (open)
        for (size_t k = from; k < h.size(); ++k) {
            float v;
            if (prefix_value(ph, h.data() + k, (int)(h.size() - k), &v)) return banked + (double)v;
        }
    return banked;
}

struct Automaton {
    std::vector<int64_t> keys;
    std::vector<int32_t> child, fail;
    std::vector<float> value, bank;
    std::vector<uint8_t> reset;
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
    std::map<Labels, int> node;
    for (int n = 0; n < N; ++n) node[label[n]] = n;
    a->fail.assign(N, 0), a->value.assign(N, 0.f), a->bank.assign(N, 0.f), a->reset.assign(N, 0);
    for (int n = 1; n < N; ++n) {
        const Labels& l = label[n];
        prefix_value(ph, l.data(), (int)l.size(), &a->value[n]);
        for (size_t k = 1; k <= l.size(); ++k)  // the longest proper suffix that is a node
            if (node.count(Labels(l.begin() + k, l.end()))) {
                a->fail[n] = node[Labels(l.begin() + k, l.end())];
                break;
            }
    }
    for (int n = 1; n < N; ++n) {
        const Labels& l = label[n];
        for (size_t k = 0; k < l.size(); ++k)  // the longest suffix, the node included, that is a phrase
            if (ph.count(Labels(l.begin() + k, l.end()))) {
                a->reset[n] = 1;
                a->bank[n] = a->value[node[Labels(l.begin() + k, l.end())]];
                break;
            }
    }
    int slots = 2;
    while (slots < 2 * N) slots *= 2;
    a->keys.assign(slots, -1), a->child.assign(slots, 0);
    const uint32_t mask = (uint32_t)slots - 1u, hmask = hash_bits >= 32 ? 0xffffffffu : (1u << hash_bits) - 1u;
    for (int n = 0; n < N; ++n)
        for (const auto& e : kids[n]) {
            uint32_t at = cb_hash(n, e.first) & hmask & mask;
            while (a->keys[at] >= 0) at = (at - 1u) & mask;
            a->keys[at] = (int64_t)(((uint64_t)n << 32) | (uint32_t)e.first);
            a->child[at] = e.second;
        }
    a->d = cn_bias_desc{a->keys.data(), a->child.data(), a->fail.data(), a->value.data(), a->bank.data(), a->reset.data(), slots, N, hash_bits, 0};
    return a;
}

struct Inputs {
    int B, Tp, V, P;
    std::unique_ptr<float[]> logp, ratio;
    std::unique_ptr<int[]> top;
};

// random log-softmax rows with the phrases and cut-off phrases lifted along the frames, so that matches, break-offs and banks occur
Inputs make_inputs(std::mt19937& rng, const Phrases& ph, int B, int Tp, int V, int P, bool foreign) {
    Inputs in{B, Tp, V, P, std::unique_ptr<float[]>(new float[(size_t)B * Tp * V]), std::unique_ptr<float[]>(new float[B]),
              std::unique_ptr<int[]>(new int[(size_t)B * Tp * (P > 0 ? P : 1)])};
    std::normal_distribution<float> gauss;
    std::vector<Labels> plant;
    for (const auto& p : ph) {
        plant.push_back(p.first);
        plant.push_back(Labels(p.first.begin(), p.first.end() - 1));
    }
    for (int b = 0; b < B; ++b) {
        Labels path;
        while ((int)path.size() < Tp) {
            if (!plant.empty())
                for (int c : plant[rng() % plant.size()]) path.push_back(c);
            path.push_back(rng() % 3 ? 0 : 1 + (int)(rng() % (V - 1)));
        }
        for (int t = 0; t < Tp; ++t) {
            float* row = in.logp.get() + ((size_t)b * Tp + t) * V;
            double z = 0;
            for (int v = 0; v < V; ++v) row[v] = gauss(rng) + (v == path[t] ? 4.f : 0.f), z += std::exp((double)row[v]);
            for (int v = 0; v < V; ++v) row[v] -= (float)std::log(z);
            std::vector<int> idx(V);
            for (int v = 0; v < V; ++v) idx[v] = v;
            std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return row[x] > row[y]; });
            for (int j = 0; j < P; ++j)
                in.top[((size_t)b * Tp + t) * P + j] = foreign && j == P - 1 && rng() % 5 == 0 ? (rng() % 2 ? V + 3 : -2) : idx[j];
        }
        in.ratio[b] = b == 1 ? 0.5f : 1.f;
    }
    return in;
}

struct Outputs {
    int W, cap;
    std::unique_ptr<int[]> hyp, hlen, nb;
    std::unique_ptr<double[]> sc, slm, pb, pnb;
    bool same_search(const Outputs& o, int B) const {  // every output but score_lm
        return !memcmp(hyp.get(), o.hyp.get(), (size_t)B * W * cap * 4) && !memcmp(hlen.get(), o.hlen.get(), (size_t)B * W * 4) &&
               !memcmp(nb.get(), o.nb.get(), (size_t)B * 4) && !memcmp(sc.get(), o.sc.get(), (size_t)B * W * 8) &&
               !memcmp(pb.get(), o.pb.get(), (size_t)B * W * 8) && !memcmp(pnb.get(), o.pnb.get(), (size_t)B * W * 8);
    }
};

Outputs outputs(int B, int W, int cap) {
    const int n = B * W;
    return Outputs{W, cap, std::unique_ptr<int[]>(new int[(size_t)n * cap]), std::unique_ptr<int[]>(new int[n]), std::unique_ptr<int[]>(new int[B]),
                   std::unique_ptr<double[]>(new double[n]), std::unique_ptr<double[]>(new double[n]), std::unique_ptr<double[]>(new double[n]),
                   std::unique_ptr<double[]>(new double[n])};
}

Outputs search(const cn_bias_desc& d, const Inputs& in, int W, double lp) {
    Outputs o = outputs(in.B, W, in.Tp + 1);
    const CtcSearchArgs a = ctc_search_args(
        ctc_beam_args(in.logp.get(), in.P > 0 ? in.top.get() : nullptr, in.ratio.get(), in.B, in.Tp, in.V, W, in.P, 0, lp,
                      ctc_beam_out(o.hyp.get(), o.cap, o.hlen.get(), o.sc.get(), o.slm.get(), o.pb.get(), o.pnb.get(), o.nb.get())),
        nullptr, 0.0, &d);
    const std::string bad = ctc_search_check(a, false);
    CHECK(bad.empty(), "%s", bad.c_str());
    if (bad.empty())
        for (int b = 0; b < in.B; ++b) ctc_search_host(a, b);
    else
        memset(o.nb.get(), 0, (size_t)in.B * 4);
    return o;
}

// the same search without automaton or state: every hypothesis keeps its labels, every candidate's score_lm is a rescan of all of them
Outputs naive(const Phrases& ph, const Inputs& in, int W, double lp) {
    struct Hyp {
        double pb, pnb, tot, slm, key;
        Labels h;
    };
    Outputs o = outputs(in.B, W, in.Tp + 1);
    for (int b = 0; b < in.B; ++b) {
        std::vector<Hyp> beam(1, Hyp{0.0, CS_LOGZERO, 0.0, 0.0, 0.0, Labels()});
        const int ssz = cs_src_size(in.ratio[b], in.Tp);
        for (int t = 0; t <= ssz && t < in.Tp; ++t) {
            const float* row = in.logp.get() + ((size_t)b * in.Tp + t) * in.V;
            if (cs_skip_frame(row[0])) continue;
            std::vector<Hyp> cand;
            for (size_t k = 0; k < beam.size(); ++k)
                for (int j = 0; j <= in.P; ++j) {
                    const Hyp& h = beam[k];
                    const int c = j == 0 ? -1 : in.top[((size_t)b * in.Tp + t) * in.P + (j - 1)];
                    const CsCand r = cs_candidate(row, in.V, 0, (int)k, j == 0, c, h.pb, h.pnb, h.h.empty() ? -1 : h.h.back(), (int)h.h.size());
                    if (r.par < 0) continue;
                    Hyp x{r.pb, r.pnb, r.tot, 0.0, 0.0, h.h};
                    if (r.tok >= 0) x.h.push_back(r.tok);
                    x.slm = rescan(ph, x.h, true);
                    x.key = cs_key(x.tot, x.slm, lp, (int)x.h.size());
                    cand.push_back(x);
                }
            std::stable_sort(cand.begin(), cand.end(), [](const Hyp& x, const Hyp& y) { return x.key > y.key; });
            if ((int)cand.size() > W) cand.resize(W);
            beam.swap(cand);
        }
        for (Hyp& h : beam) h.slm = rescan(ph, h.h, false), h.key = cs_key(h.tot, h.slm, lp, (int)h.h.size());
        std::stable_sort(beam.begin(), beam.end(), [](const Hyp& x, const Hyp& y) { return x.key > y.key; });
        o.nb[b] = (int)beam.size();
        for (int r = 0; r < W; ++r) {
            const int s = b * W + r;
            int* row = o.hyp.get() + (size_t)s * o.cap;
            for (int i = 0; i < o.cap; ++i) row[i] = 0;
            if (r < (int)beam.size()) {
                std::copy(beam[r].h.begin(), beam[r].h.end(), row);
                o.hlen[s] = (int)beam[r].h.size(), o.sc[s] = beam[r].tot, o.slm[s] = beam[r].slm, o.pb[s] = beam[r].pb, o.pnb[s] = beam[r].pnb;
            } else {
                o.hlen[s] = 0, o.sc[s] = o.pb[s] = o.pnb[s] = CS_LOGZERO, o.slm[s] = 0.0;
            }
        }
    }
    return o;
}

int banks_seen = 0;

void check_search(const Phrases& ph, int hash_bits, std::mt19937& rng, int B, int Tp, int V, int W, int P, double lp, bool foreign) {
    const auto a = build(ph, hash_bits);
    const Inputs in = make_inputs(rng, ph, B, Tp, V, P, foreign);
    const Outputs o = search(a->d, in, W, lp), n = naive(ph, in, W, lp);
    CHECK(o.same_search(n, B) && !memcmp(o.slm.get(), n.slm.get(), (size_t)B * W * 8), "Tp %d W %d P %d bits %d: the search is not the naive one", Tp, W,
          P, hash_bits);
    for (int b = 0; b < B; ++b) {
        CHECK(o.nb[b] >= 1 && o.nb[b] <= W, "nbeam %d", o.nb[b]);
        double prev = 0;
        for (int j = 0; j < o.nb[b]; ++j) {
            const int s = b * W + j, len = o.hlen[s];
            CHECK(len >= 0 && len <= Tp, "length %d", len);
            const int* h = o.hyp.get() + (size_t)s * o.cap;
            for (int i = 0; i < len; ++i) CHECK(h[i] > 0 && h[i] < V, "label %d", h[i]);
            banks_seen += o.slm[s] != 0.0;
            const double key = (o.sc[s] + o.slm[s]) + lp * len;
            CHECK(j == 0 || key <= prev, "beam not sorted");
            prev = key;
        }
    }
}

}  // namespace

int main() {
    std::mt19937 rng(2024);
    const int V = 12;
    Labels longest;
    for (int i = 0; i < CB_MAX_PHRASE; ++i) longest.push_back(1 + i % 5 + (i % 2) * 5);
    const std::vector<Phrases> sets = {
        {},
        {{{3}, 2.f}},
        {{{1, 2, 3}, 2.f}, {{1, 4}, 3.f}, {{1, 2, 5}, 0.5f}, {{6, 1, 2}, 2.f}},
        {{{1, 2, 3, 4}, 2.f}, {{2, 3}, 3.f}, {{6, 1, 2}, 0.5f}},
        {{{6, 1}, 2.f}, {{6, 1, 2}, 3.f}, {{1, 4}, 0.5f}},
        {{{1, 2, 2, 3}, 2.f}, {{2, 3, 3}, 3.f}, {{3, 3}, 0.5f}},
        {{longest, 0.5f}, {{6, 1, 2}, 2.f}},
        {{{1, 4}, -1.f}, {{6, 1, 2}, -1.f}, {{7, 3}, 2.f}},
    };
    for (const Phrases& ph : sets)
        for (int bits : {32, 1, 0}) {
            for (int Tp : {1, 12, 40}) {
                check_search(ph, bits, rng, 3, Tp, V, 1, 1, 0.0, false);
                check_search(ph, bits, rng, 3, Tp, V, 2, 0, 0.3, false);
                check_search(ph, bits, rng, 3, Tp, V, 5, 3, 0.25, true);
                check_search(ph, bits, rng, 3, Tp, V, 32, 8, 0.25, true);
                check_search(ph, bits, rng, 2, Tp, V, 32, V - 1, 0.0, false);
            }
        }
    CHECK(banks_seen > 1000, "only %d hypotheses with a bonus", banks_seen);
    {  // the root alone: with tables, without tables, with no node at all - the same bytes, score_lm 0
        const auto empty = build(Phrases(), 32);
        const Inputs in = make_inputs(rng, sets[2], 3, 40, V, 8, true);
        cn_bias_desc bare = {};
        bare.slots = 1, bare.nodes = 1, bare.hash_bits = 32;
        const Outputs x = search(empty->d, in, 32, 0.25), y = search(bare, in, 32, 0.25);
        bare.nodes = 0;
        const Outputs z = search(bare, in, 32, 0.25);
        CHECK(x.same_search(y, 3) && x.same_search(z, 3), "the root alone depends on its descriptor");
        for (int i = 0; i < 3 * 32; ++i) CHECK(x.slm[i] == 0.0 && y.slm[i] == 0.0 && z.slm[i] == 0.0, "score_lm with the root alone");
    }
    {  // refusals
        const auto a = build(sets[2], 32);
        CHECK(!ctc_search_check(ctc_search_args(CtcBeamArgs(), nullptr, 0.0, &a->d), false).empty(), "null arguments accepted");
        cn_bias_desc d = a->d;
        d.slots = 3;
        CHECK(!cb_check_desc(d).empty(), "a slot count that is no power of two accepted");
        d = a->d, d.nodes = -1;
        CHECK(!cb_check_desc(d).empty(), "a negative node count accepted");
        d = a->d, d.fail = nullptr;
        CHECK(!cb_check_desc(d).empty(), "a null table accepted");
        d = a->d, d.hash_bits = 33;
        CHECK(!cb_check_desc(d).empty(), "hash_bits 33 accepted");
        CHECK(cb_check_desc(a->d).empty(), "a good descriptor refused");
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ctc_bias_check: all checks held\n");
    return 0;
}
