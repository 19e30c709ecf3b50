// Stand-alone host check of the CTC prefix beam search that merges candidates by prefix: the functions and the serial search the
// library and its kernel are built from (csrc/ctc_search_host.h over csrc/ctc_search.h and csrc/ctc_merge_search.h) run on the CPU on
// random log-posteriors made in memory, every array a heap block of exactly the size the search was told.  Checked:
//   * ctc_search_host with `merge` set gives the bytes of a naive search that keeps every hypothesis' labels in a map from label sequence to
//     (p_blk, p_nblk): hypotheses, order, lengths and all scores; pruned lists with duplicate labels, blanks and ids outside [0, V),
//     size ratios that cut frames, frames that are skipped, beams up to 32 x 32;
//   * the kept hypotheses spell pairwise different sequences, lengths and labels are in range;
//   * the kernel's identity test - ids, hash, and cm_same_sequence on the back-pointer chains - decides every (extension, kept
//     hypothesis) pair of every frame as the comparison of the label vectors does, and so does cm_same_sequence alone; the runs
//     contain folds into hypotheses whose prefix was dropped and made again (counted);
//   * the empty bias descriptor (with the root alone) gives the LM-free bytes;
//   * with beam 1 or pruning 0 the fold has nothing to do: the bytes are those of the same function with `merge` off (and the root
//     alone as its bias descriptor);
//   * the refusals refuse.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/ctc_merge_check.cpp -o ctc_merge_check
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

struct Case {
    int B, Tp, V, W, P, blank;
    double lp;
    std::unique_ptr<float[]> logp, ratio;
    std::unique_ptr<int[]> top;
};

struct Out {
    int B, W, cap;
    std::unique_ptr<int[]> hyp, len, nb;
    std::unique_ptr<double[]> sc, slm, pb, pnb;
    Out(int B_, int W_, int cap_) : B(B_), W(W_), cap(cap_), hyp(new int[(size_t)B_ * W_ * cap_]), len(new int[(size_t)B_ * W_]), nb(new int[B_]),
                                    sc(new double[(size_t)B_ * W_]), slm(new double[(size_t)B_ * W_]), pb(new double[(size_t)B_ * W_]),
                                    pnb(new double[(size_t)B_ * W_]) {
        std::fill(hyp.get(), hyp.get() + (size_t)B * W * cap, -7);
        std::fill(len.get(), len.get() + (size_t)B * W, -7);
        std::fill(nb.get(), nb.get() + B, -7);
        for (double* a : {sc.get(), slm.get(), pb.get(), pnb.get()}) std::fill(a, a + (size_t)B * W, -7.5);
    }
    CtcBeamOut view() { return ctc_beam_out(hyp.get(), cap, len.get(), sc.get(), slm.get(), pb.get(), pnb.get(), nb.get()); }
    bool same(const Out& o) const {
        return !memcmp(hyp.get(), o.hyp.get(), (size_t)B * W * cap * 4) && !memcmp(len.get(), o.len.get(), (size_t)B * W * 4) &&
               !memcmp(nb.get(), o.nb.get(), (size_t)B * 4) && !memcmp(sc.get(), o.sc.get(), (size_t)B * W * 8) &&
               !memcmp(slm.get(), o.slm.get(), (size_t)B * W * 8) && !memcmp(pb.get(), o.pb.get(), (size_t)B * W * 8) &&
               !memcmp(pnb.get(), o.pnb.get(), (size_t)B * W * 8);
    }
};

// labels: how many labels beside the blank share the mass (0: all of them); odd: pruned lists with duplicates, blanks and foreign ids
Case make_case(std::mt19937& rng, int B, int Tp, int V, int W, int P, int labels, bool odd, double lp) {
    Case c;
    c.B = B, c.Tp = Tp, c.V = V, c.W = W, c.P = P, c.blank = 0, c.lp = lp;
    c.logp.reset(new float[(size_t)B * Tp * V]);
    c.ratio.reset(new float[B]);
    c.top.reset(new int[(size_t)B * Tp * P + 1]);
    std::normal_distribution<float> nd(0.f, 2.f);
    for (int b = 0; b < B; ++b) {
        c.ratio[b] = b % 3 == 1 ? 0.6f : 1.f;
        for (int t = 0; t < Tp; ++t) {
            float* row = c.logp.get() + ((size_t)b * Tp + t) * V;
            double sum = 0.0;
            for (int v = 0; v < V; ++v) {
                row[v] = (labels == 0 || v <= labels) ? nd(rng) : -12.f + 0.001f * (float)v;
                if (v == 0 && rng() % 7 == 0) row[v] += 8.f;  // a frame that is (nearly) all blank: skipped
                sum += std::exp((double)row[v]);
            }
            for (int v = 0; v < V; ++v) row[v] = (float)((double)row[v] - std::log(sum));
            std::vector<int> order(V);
            for (int v = 0; v < V; ++v) order[v] = v;
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return row[x] > row[y]; });
            int* top = c.top.get() + ((size_t)b * Tp + t) * P;
            for (int j = 0; j < P; ++j) top[j] = order[j % V];
            if (odd)
                for (int j = 0; j < P; ++j) {
                    const unsigned r = rng() % 8;
                    if (r == 0 && j > 0) top[j] = top[rng() % j];  // a label twice
                    if (r == 1) top[j] = V + (int)(rng() % 3);
                    if (r == 2) top[j] = -1 - (int)(rng() % 3);
                }
        }
    }
    return c;
}

cn_bias_desc no_bias() {  // the root alone: a valid descriptor whose tables are not read
    cn_bias_desc d = {};
    d.slots = 1, d.nodes = 0, d.hash_bits = 32;
    return d;
}

CtcSearchArgs args_of(const Case& c, Out& o, const cn_bias_desc* bias, bool merge = true) {
    return ctc_search_args(ctc_beam_args(c.logp.get(), c.P ? c.top.get() : nullptr, c.ratio.get(), c.B, c.Tp, c.V, c.W, c.P, c.blank, c.lp, o.view()),
                           nullptr, 0.0, bias, merge);
}

struct Stats {
    long folds = 0, relinked = 0, pairs = 0, walks = 0;
};

// The naive search of utterance b: the kept hypotheses are a map from label sequence to (p_blk, p_nblk) plus the beam's order; a
// frame's candidates are gathered into a new map (first the stays, then every extension: added to the entry its labels have, or a new
// entry), then ordered.  Beside it the kernel's identity state (ids, hashes, back-pointers) is kept and asked about every pair.
void naive(const Case& c, int b, Out& o, Stats* st) {
    struct Hyp {
        double pb, pnb;
        int id, pfx;
        uint32_t hash;
    };
    struct Cand {
        Labels seq;
        double pb, pnb, tot, key;
        int par, tok;
    };
    const int W = c.W, P = c.P, V = c.V;
    std::map<Labels, Hyp> kept;
    std::vector<Labels> order(1);
    kept[Labels()] = Hyp{0.0, CS_LOGZERO, 0, -1, 0u};
    std::vector<unsigned char> hpar((size_t)c.Tp * W);
    std::vector<int> htok((size_t)c.Tp * W);
    const float* logp = c.logp.get() + (size_t)b * c.Tp * V;
    const int ssz = cs_src_size(c.ratio[b], c.Tp);
    int steps = 0;
    for (int t = 0; t < c.Tp && t <= ssz; ++t) {
        const float* row = logp + (size_t)t * V;
        if ((double)(float)std::exp((double)row[c.blank]) > 0.95) continue;
        Labels labs;
        for (int j = 0; j < P; ++j) {
            const int l = c.top[((size_t)b * c.Tp + t) * P + j];
            if (l >= 0 && l < V && l != c.blank && std::find(labs.begin(), labs.end(), l) == labs.end()) labs.push_back(l);
        }
        std::vector<Cand> cand;
        std::map<Labels, int> at;  // sequence -> its entry in cand
        for (int k = 0; k < (int)order.size(); ++k) {
            const Labels& s = order[k];
            const Hyp& h = kept[s];
            Cand x;
            x.seq = s, x.par = k, x.tok = -1;
            const double pt = (double)row[c.blank];
            x.pb = cs_logaddexp(h.pb + pt, h.pnb + pt);
            x.pnb = s.empty() ? CS_LOGZERO : h.pnb + (double)row[s.back()];
            at[s] = (int)cand.size();
            cand.push_back(x);
        }
        for (int k = 0; k < (int)order.size(); ++k) {
            const Labels s = order[k];
            const Hyp h = kept[s];
            for (int l : labs) {
                const double pt = (double)row[l];
                const double pnb = (!s.empty() && s.back() == l) ? h.pb + pt : cs_logaddexp(h.pb + pt, h.pnb + pt);
                Labels s2 = s;
                s2.push_back(l);
                // the kernel's identity test on every kept hypothesis, against the comparison of the vectors
                for (int kp = 0; kp < (int)order.size(); ++kp) {
                    const Labels& sp = order[kp];
                    const Hyp& hp = kept[sp];
                    if (sp.size() != s2.size() || sp.back() != l) continue;
                    const bool truth = sp == s2;
                    const bool walk = cm_same_sequence(hpar.data(), htok.data(), W, steps, kp, k, l);
                    const bool device = hp.pfx == h.id || (hp.hash == cm_hash(h.hash, l) && walk);
                    CHECK(walk == truth && device == truth, "identity: frame %d, (%d, %d) against %d: walk %d device %d truth %d", t, k, l, kp,
                          (int)walk, (int)device, (int)truth);
                    ++st->pairs;
                    st->walks += hp.pfx != h.id;
                    if (truth) {
                        ++st->folds;
                        st->relinked += hp.pfx != h.id;
                    }
                }
                if (at.count(s2)) {
                    Cand& stay = cand[at[s2]];
                    CHECK(stay.tok == -1, "two extensions spell one sequence");
                    stay.pnb = cs_logaddexp(stay.pnb, pnb);
                } else {
                    Cand x;
                    x.seq = s2, x.par = k, x.tok = l, x.pb = CS_LOGZERO, x.pnb = pnb;
                    cand.push_back(x);  // (no entry in `at`: only kept sequences take folds; an extension's labels are its own)
                }
            }
        }
        // the reference's candidate order: per kept hypothesis its stay, then its extensions in list order
        std::vector<int> idx;
        for (int k = 0; k < (int)order.size(); ++k)
            for (int i = 0; i < (int)cand.size(); ++i)
                if (cand[i].par == k) idx.push_back(i);  // (the stays stand first in `cand`)
        for (int i : idx) {
            Cand& x = cand[i];
            x.tot = cs_logaddexp(x.pb, x.pnb);
            x.key = cs_key(x.tot, 0.0, c.lp, (int)x.seq.size());
        }
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return cand[x].key > cand[y].key; });
        if ((int)idx.size() > W) idx.resize(W);
        std::map<Labels, Hyp> next;
        std::vector<Labels> norder;
        for (int r = 0; r < (int)idx.size(); ++r) {
            const Cand& x = cand[idx[r]];
            const Hyp& par = kept[order[x.par]];
            CHECK(!next.count(x.seq), "a sequence is kept twice");
            next[x.seq] = x.tok < 0 ? Hyp{x.pb, x.pnb, par.id, par.pfx, par.hash} : Hyp{x.pb, x.pnb, steps * W + r + 1, par.id, cm_hash(par.hash, x.tok)};
            norder.push_back(x.seq);
            hpar[(size_t)steps * W + r] = (unsigned char)x.par;
            htok[(size_t)steps * W + r] = x.tok;
        }
        kept.swap(next);
        order.swap(norder);
        ++steps;
    }
    o.nb[b] = (int)order.size();
    for (int r = 0; r < W; ++r) {
        const size_t row = (size_t)b * W + r;
        std::fill(o.hyp.get() + row * o.cap, o.hyp.get() + (row + 1) * o.cap, 0);
        o.len[row] = 0, o.slm[row] = 0.0;
        o.sc[row] = o.pb[row] = o.pnb[row] = CS_LOGZERO;
        if (r < (int)order.size()) {
            const Hyp& h = kept[order[r]];
            std::copy(order[r].begin(), order[r].end(), o.hyp.get() + row * o.cap);
            o.len[row] = (int)order[r].size();
            o.pb[row] = h.pb, o.pnb[row] = h.pnb, o.sc[row] = cs_logaddexp(h.pb, h.pnb);
        }
    }
}

void check_case(const Case& c, Stats* st) {
    const int cap = c.Tp + 1;
    Out got(c.B, c.W, cap), want(c.B, c.W, cap), empty(c.B, c.W, cap);
    const CtcSearchArgs a = args_of(c, got, nullptr);
    CHECK(ctc_search_check(a, false).empty(), "ctc_search_check: %s", ctc_search_check(a, false).c_str());
    const cn_bias_desc root = no_bias();
    const CtcSearchArgs ae = args_of(c, empty, &root);
    for (int b = 0; b < c.B; ++b) {
        ctc_search_host(a, b);
        ctc_search_host(ae, b);
        naive(c, b, want, st);
    }
    CHECK(got.same(want), "host search and naive search differ (T' %d, %d / %d)", c.Tp, c.W, c.P);
    CHECK(got.same(empty), "the empty bias descriptor changes the result (T' %d, %d / %d)", c.Tp, c.W, c.P);
    for (int b = 0; b < c.B; ++b) {
        CHECK(got.nb[b] >= 1 && got.nb[b] <= c.W, "nbeam out of range");
        std::map<Labels, int> seen;
        for (int r = 0; r < got.nb[b] && r < c.W; ++r) {
            const size_t row = (size_t)b * c.W + r;
            const int n = got.len[row];
            CHECK(n >= 0 && n < cap, "length out of range");
            Labels l(got.hyp.get() + row * cap, got.hyp.get() + row * cap + std::max(0, std::min(n, cap)));
            for (int x : l) CHECK(x > 0 && x < c.V, "label out of range");
            CHECK(++seen[l] == 1, "a sequence is kept twice");
            if (r > 0) CHECK(cs_key(got.sc[row - 1], 0.0, c.lp, got.len[row - 1]) >= cs_key(got.sc[row], 0.0, c.lp, n), "beam not sorted");
        }
    }
    if (c.W == 1 || c.P == 0) {  // nothing can fold: the unmerged search (the odd lists apart, whose duplicates it would take twice)
        Out plain(c.B, c.W, cap);
        const CtcSearchArgs ab = args_of(c, plain, &root, false);
        for (int b = 0; b < c.B; ++b) ctc_search_host(ab, b);
        CHECK(got.same(plain), "beam %d pruning %d: not the unmerged search", c.W, c.P);
    }
}

void check_refusals() {
    std::mt19937 rng(5);
    Case c = make_case(rng, 2, 6, 5, 3, 2, 0, false, 0.0);
    Out o(c.B, c.W, c.Tp + 1);
    CtcSearchArgs a = args_of(c, o, nullptr);
    cn_ngram_desc ng = {};
    cn_bias_desc root = no_bias();
    CtcSearchArgs x = a;
    x.ng = &ng, x.bias = &root;
    CHECK(ctc_search_check(x, false).find("at most one") != std::string::npos, "both descriptors must be refused");
    x = a, x.W = 33;
    CHECK(!ctc_search_check(x, false).empty(), "beam 33");
    x = a, x.P = -1;
    CHECK(!ctc_search_check(x, false).empty(), "pruning -1");
    x = a, x.logp = nullptr;
    CHECK(!ctc_search_check(x, false).empty(), "null logp");
    x = a, x.out.score_lm = nullptr;
    CHECK(!ctc_search_check(x, false).empty(), "null score_lm");
    x = a, x.out.Lmax = c.Tp;
    CHECK(!ctc_search_check(x, false).empty(), "hyp_cap");
    x = a, x.blank = c.V;
    CHECK(!ctc_search_check(x, false).empty(), "blank");
    x = a, x.lp = std::nan("");
    CHECK(!ctc_search_check(x, false).empty(), "length_penalty");
    CHECK(!ctc_search_check(a, true).empty(), "missing scratch must be refused where it is needed");
    cn_bias_desc odd = root;
    odd.slots = 3;
    x = a, x.bias = &odd;
    CHECK(!ctc_search_check(x, false).empty(), "slot count");
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    Stats st;
    const int beams[][2] = {{1, 3}, {3, 0}, {1, 0}, {2, 2}, {3, 3}, {5, 8}, {20, 30}, {32, 32}};
    for (const auto& wp : beams)
        for (int Tp : {1, 2, 7, 24})
            for (int labels : {2, 3, 0})
                for (int odd = 0; odd < 2; ++odd) {
                    if ((wp[0] == 1 || wp[1] == 0) && odd) continue;  // (the unmerged search has no rule for duplicate labels)
                    Case c = make_case(rng, 3, Tp, 12, wp[0], wp[1], labels, odd != 0, labels == 3 ? 0.3 : 0.0);
                    check_case(c, &st);
                }
    {
        Case c = make_case(rng, 2, 60, 40, 32, 32, 3, true, 0.1);  // more than 256 candidates a frame, long chains
        check_case(c, &st);
    }
    check_refusals();
    CHECK(st.folds > 1000 && st.relinked > 10 && st.walks > st.relinked, "the runs do not cover the fold: %ld folds, %ld relinked, %ld walks", st.folds,
          st.relinked, st.walks);
    printf("ctc_merge_check: %ld pairs, %ld folds, %ld of them into a hypothesis whose prefix was made again, %ld chain walks; %d failures\n", st.pairs,
           st.folds, st.relinked, st.walks, failures);
    return failures ? 1 : 0;
}
