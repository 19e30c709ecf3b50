// Stand-alone host check of the CTC prefix beam search with word n-gram fusion: the scoring core (csrc/ngram_core.h) and the step
// functions and serial search the library and its kernels are built from (csrc/ctc_search.h, csrc/ctc_ngram_search.h, csrc/ctc_search_host.h)
// run on the CPU, on a small n-gram
// model and random log-posteriors made in memory, every array a heap block of exactly the size the search was told.  Checked:
//   * the word score put together from independent probes (ng_probe / ng_probe_score) has ng_word_score's bits;
//   * every returned score_lm is lm_scale times the word scores of the hypothesis' words, glued and summed as the ranker does
//     (dyadic model values and a power-of-two lm_scale: exactly);
//   * the beam comes back sorted by its key, lengths and labels are in range, and the refusals refuse;
//   * with lm_scale = 0 - the search without a language model, through the same functions - every output but score_lm (0) is the same
//     bytes whatever the n-gram model;
//   * a pruned label outside [0, V) makes no candidate: the outputs are the bytes of the run with the blank in its place.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc -I tools tools/ctc_ngram_check.cpp -o ctc_ngram_check
// Exit status 0 when every check held.
#include "ngram_check_model.h"

#include "ctc_search_host.h"

namespace {

// the ranker's row score (ngram.hip: ng_score_row_host with drop_id 2), summed in float64 as the search does
double row_score(const cn_ngram_desc& d, const int* tok, int n, double lm_scale) {
    int32_t ids[NG_HIST + 1];
    for (int i = 0; i < NG_HIST; ++i) ids[i] = d.bos;
    int before = 0;
    double acc = 0.0;
    auto word = [&](int32_t w) {
        const int c = before + 1 < d.order - 1 ? before + 1 : d.order - 1;
        acc += (double)ng_word_score(d, ids + NG_HIST, c, w) * lm_scale;
        for (int i = 0; i + 1 < NG_HIST; ++i) ids[i] = ids[i + 1];
        ids[NG_HIST - 1] = w;
        ++before;
    };
    NgPiece carry = ng_piece(d, 0, false);
    for (int i = 0; i < n; ++i) {
        const bool real = tok[i] != CG_DROP;
        const NgPiece pc = ng_piece(d, tok[i], real);
        if (real && pc.starts && carry.pw != 1) word(ng_word_id(d, carry.h));
        carry = ng_combine(carry, pc);
    }
    if (carry.pw != 1) word(ng_word_id(d, carry.h));
    word(d.eos);
    return acc;
}

void check_probes(const Model& m, std::mt19937& rng, int n_ids) {
    for (int it = 0; it < 2000; ++it) {
        int32_t hist[NG_HIST];
        for (int i = 0; i < NG_HIST; ++i) hist[i] = (int)(rng() % n_ids);
        const int c = (int)(rng() % m.d.order), w = (int)(rng() % n_ids);
        NgProbe pr[NG_TASKS];
        for (int t = 0; t < NG_TASKS - 1; ++t) ng_probe(m.d, hist + NG_HIST, c, w, t, &pr[t]);
        const float a = ng_probe_score(pr, c), b = ng_word_score(m.d, hist + NG_HIST, c, w);
        CHECK(memcmp(&a, &b, 4) == 0, "order %d c %d: probes %a, core %a", m.d.order, c, a, b);
    }
}

struct Inputs {
    int B, Tp, V, P;
    std::unique_ptr<float[]> logp, ratio;
    std::unique_ptr<int[]> top;
};

Inputs make_inputs(std::mt19937& rng, int B, int Tp, int V, int P) {
    Inputs in{B, Tp, V, P, std::unique_ptr<float[]>(new float[(size_t)B * Tp * V]), std::unique_ptr<float[]>(new float[B]),
              std::unique_ptr<int[]>(new int[(size_t)B * Tp * (P > 0 ? P : 1)])};
    std::normal_distribution<float> gauss;
    for (int r = 0; r < B * Tp; ++r) {
        float* row = in.logp.get() + (size_t)r * V;
        double z = 0;
        for (int v = 0; v < V; ++v) row[v] = 2.f * gauss(rng), z += std::exp((double)row[v]);
        for (int v = 0; v < V; ++v) row[v] -= (float)std::log(z);
        std::vector<int> idx(V);
        for (int v = 0; v < V; ++v) idx[v] = v;
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return row[x] > row[y]; });
        for (int j = 0; j < P; ++j) in.top[(size_t)r * P + j] = j == P - 1 && rng() % 7 == 0 ? V + 3 : idx[j];  // (some labels outside [0, V))
    }
    for (int b = 0; b < B; ++b) in.ratio[b] = b == 1 ? 0.5f : 1.f;
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

Outputs search(const Model& m, const Inputs& in, int W, double lp, double lm_scale) {
    const int B = in.B, n = B * W, cap = in.Tp + 1;
    Outputs o{W, cap, std::unique_ptr<int[]>(new int[(size_t)n * cap]), std::unique_ptr<int[]>(new int[n]), std::unique_ptr<int[]>(new int[B]),
              std::unique_ptr<double[]>(new double[n]), std::unique_ptr<double[]>(new double[n]), std::unique_ptr<double[]>(new double[n]),
              std::unique_ptr<double[]>(new double[n])};
    const CtcSearchArgs a = ctc_search_args(
        ctc_beam_args(in.logp.get(), in.P > 0 ? in.top.get() : nullptr, in.ratio.get(), B, in.Tp, in.V, W, in.P, 0, lp,
                      ctc_beam_out(o.hyp.get(), cap, o.hlen.get(), o.sc.get(), o.slm.get(), o.pb.get(), o.pnb.get(), o.nb.get())),
        &m.d, lm_scale);
    const std::string bad = ctc_search_check(a, false);
    CHECK(bad.empty(), "%s", bad.c_str());
    if (bad.empty())
        for (int b = 0; b < B; ++b) ctc_search_host(a, b);
    else
        memset(o.nb.get(), 0, (size_t)B * 4);
    return o;
}

void check_search(const Model& m, std::mt19937& rng, int B, int Tp, int W, int P, double lp, double lm_scale) {
    const int V = m.d.vocab, cap = Tp + 1;
    const Inputs in = make_inputs(rng, B, Tp, V, P);
    const Outputs o = search(m, in, W, lp, lm_scale);
    for (int b = 0; b < B; ++b) {
        CHECK(o.nb[b] >= 1 && o.nb[b] <= W, "nbeam %d", o.nb[b]);
        double prev = 0;
        for (int j = 0; j < o.nb[b]; ++j) {
            const int s = b * W + j, n = o.hlen[s];
            CHECK(n >= 0 && n <= Tp, "length %d", n);
            const int* h = o.hyp.get() + (size_t)s * cap;
            for (int i = 0; i < n; ++i) CHECK(h[i] > 0 && h[i] < V, "label %d", h[i]);
            const double want = row_score(m.d, h, n, lm_scale);
            CHECK(o.slm[s] == want, "order %d W %d P %d utt %d beam %d: score_lm %a, words %a", m.d.order, W, P, b, j, o.slm[s], want);
            const double key = (o.sc[s] + o.slm[s]) + lp * n;
            CHECK(j == 0 || key <= prev, "beam not sorted");
            prev = key;
        }
    }
}

// lm_scale = 0 is the search without a language model: the n-gram model `other` (same pieces, another order) changes no output
void check_no_lm(const Model& m, const Model& other, std::mt19937& rng, int Tp, int W, int P, double lp) {
    const Inputs in = make_inputs(rng, 3, Tp, m.d.vocab, P);
    const Outputs x = search(m, in, W, lp, 0.0), y = search(other, in, W, lp, 0.0);
    CHECK(x.same_search(y, 3), "Tp %d W %d P %d: the search with lm_scale 0 depends on the n-gram model", Tp, W, P);
    for (int i = 0; i < 3 * W; ++i) CHECK(x.slm[i] == 0.0 && y.slm[i] == 0.0, "score_lm %a / %a with lm_scale 0", x.slm[i], y.slm[i]);
}

// a label outside [0, V) in the middle of every frame's pruned list (negative, V itself, far outside) is no candidate, as the blank
void check_foreign(const Model& m, std::mt19937& rng, int Tp, int W, int P, double lp, double lm_scale) {
    Inputs in = make_inputs(rng, 3, Tp, m.d.vocab, P);
    const int foreign[] = {-1, in.V, -2000000000, 2000000000};
    for (int r = 0; r < 3 * Tp; ++r) in.top[(size_t)r * P + P / 2] = foreign[r % 4];
    const Outputs x = search(m, in, W, lp, lm_scale);
    for (int r = 0; r < 3 * Tp; ++r) in.top[(size_t)r * P + P / 2] = 0;  // the blank
    const Outputs y = search(m, in, W, lp, lm_scale);
    CHECK(x.same_search(y, 3) && !memcmp(x.slm.get(), y.slm.get(), (size_t)3 * W * 8), "Tp %d W %d P %d: a foreign label changed the search", Tp, W, P);
    for (int b = 0; b < 3; ++b)
        for (int j = 0; j < x.nb[b]; ++j)
            for (int i = 0; i < x.hlen[b * W + j]; ++i) {
                const int t = x.hyp[((size_t)b * W + j) * x.cap + i];
                CHECK(t > 0 && t < in.V, "label %d", t);
            }
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    const std::vector<std::string> words = {"ab", "ba", "abc", "c", "cc", "bca", "a", "b", "cab", "bb", "abcbc", "bc"};
    std::vector<std::string> pieces;
    std::vector<uint8_t> starts;
    const auto first = make_model(4, rng, words, &pieces, &starts);
    for (int order : {1, 2, 3, 5, 8}) {
        const auto m = make_model(order, rng, words, &pieces, &starts);
        check_probes(*m, rng, (int)words.size() + 3);
        for (int Tp : {1, 12, 40}) {
            check_search(*m, rng, 3, Tp, 1, 1, 0.0, 0.5);
            check_search(*m, rng, 3, Tp, 2, 0, 0.3, 0.5);
            check_search(*m, rng, 3, Tp, 5, 3, 0.25, 2.0);
            check_search(*m, rng, 3, Tp, 32, 8, 0.25, 0.5);
            check_search(*m, rng, 2, Tp, 32, 32 < m->d.vocab - 1 ? 32 : m->d.vocab - 1, 0.0, 0.0);
        }
        check_no_lm(*m, *first, rng, 12, 5, 3, 0.25);
        check_no_lm(*m, *first, rng, 40, 32, 8, 0.3);
        check_foreign(*m, rng, 12, 5, 3, 0.25, 0.5);
        check_foreign(*m, rng, 40, 32, 8, 0.3, 0.0);
        // refusals
        CHECK(!ctc_search_check(ctc_search_args(CtcBeamArgs(), &m->d, 0.5), false).empty(), "null arguments accepted");
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ctc_ngram_check: all checks held\n");
    return 0;
}
