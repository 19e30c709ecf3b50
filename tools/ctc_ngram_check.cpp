// Stand-alone host check of the CTC prefix beam search with word n-gram fusion: the scoring core (csrc/ngram_core.h) and the step
// functions and serial search the library and its kernel are built from (csrc/ctc_ngram_search.h) run on the CPU, on a small n-gram
// model and random log-posteriors made in memory, every array a heap block of exactly the size the search was told.  Checked:
//   * the word score put together from independent probes (cg_probe / cg_word_score) has ng_word_score's bits;
//   * every returned score_lm is lm_scale times the word scores of the hypothesis' words, glued and summed as the ranker does
//     (dyadic model values and a power-of-two lm_scale: exactly);
//   * the beam comes back sorted by its key, lengths and labels are in range, and the refusals refuse.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc -I tools tools/ctc_ngram_check.cpp -o ctc_ngram_check
// Exit status 0 when every check held.
#include "ngram_check_model.h"

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
        NgProbe pr[CG_TASKS];
        for (int t = 0; t < CG_TASKS - 1; ++t) cg_probe(m.d, hist + NG_HIST, c, w, t, &pr[t]);
        const float a = cg_word_score(pr, c), b = ng_word_score(m.d, hist + NG_HIST, c, w);
        CHECK(memcmp(&a, &b, 4) == 0, "order %d c %d: probes %a, core %a", m.d.order, c, a, b);
    }
}

void check_search(const Model& m, std::mt19937& rng, int B, int Tp, int W, int P, double lp, double lm_scale) {
    const int V = m.d.vocab, cap = Tp + 1;
    std::unique_ptr<float[]> logp(new float[(size_t)B * Tp * V]), ratio(new float[B]);
    std::unique_ptr<int[]> top(new int[(size_t)B * Tp * (P > 0 ? P : 1)]);
    std::normal_distribution<float> gauss;
    for (int r = 0; r < B * Tp; ++r) {
        float* row = logp.get() + (size_t)r * V;
        double z = 0;
        for (int v = 0; v < V; ++v) row[v] = 2.f * gauss(rng), z += std::exp((double)row[v]);
        for (int v = 0; v < V; ++v) row[v] -= (float)std::log(z);
        std::vector<int> idx(V);
        for (int v = 0; v < V; ++v) idx[v] = v;
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return row[x] > row[y]; });
        for (int j = 0; j < P; ++j) top[(size_t)r * P + j] = j == P - 1 && rng() % 7 == 0 ? V + 3 : idx[j];  // (some labels outside [0, V))
    }
    for (int b = 0; b < B; ++b) ratio[b] = b == 1 ? 0.5f : 1.f;
    std::unique_ptr<int[]> hyp(new int[(size_t)B * W * cap]), hlen(new int[B * W]), nb(new int[B]);
    std::unique_ptr<double[]> sc(new double[B * W]), slm(new double[B * W]), pb(new double[B * W]), pnb(new double[B * W]);
    CtcNgramArgs a;
    a.d = m.d;
    a.logp = logp.get(), a.top_idx = P > 0 ? top.get() : nullptr, a.size_ratio = ratio.get();
    a.B = B, a.Tp = Tp, a.V = V, a.P = P, a.W = W, a.blank = 0, a.Lmax = cap, a.lp = lp, a.lm_scale = lm_scale;
    a.hyp = hyp.get(), a.hyp_len = hlen.get(), a.score = sc.get(), a.score_lm = slm.get(), a.p_blk = pb.get(), a.p_nblk = pnb.get();
    a.n_out = nb.get();
    const std::string bad = cg_check(a, false);
    CHECK(bad.empty(), "%s", bad.c_str());
    if (!bad.empty()) return;
    for (int b = 0; b < B; ++b) cg_search_host(a, b);
    for (int b = 0; b < B; ++b) {
        CHECK(nb[b] >= 1 && nb[b] <= W, "nbeam %d", nb[b]);
        double prev = 0;
        for (int j = 0; j < nb[b]; ++j) {
            const int o = b * W + j, n = hlen[o];
            CHECK(n >= 0 && n <= Tp, "length %d", n);
            const int* h = hyp.get() + (size_t)o * cap;
            for (int i = 0; i < n; ++i) CHECK(h[i] > 0 && h[i] < V, "label %d", h[i]);
            const double want = row_score(m.d, h, n, lm_scale);
            CHECK(slm[o] == want, "order %d W %d P %d utt %d beam %d: score_lm %a, words %a", m.d.order, W, P, b, j, slm[o], want);
            const double key = (sc[o] + slm[o]) + lp * n;
            CHECK(j == 0 || key <= prev, "beam not sorted");
            prev = key;
        }
    }
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    const std::vector<std::string> words = {"ab", "ba", "abc", "c", "cc", "bca", "a", "b", "cab", "bb", "abcbc", "bc"};
    for (int order : {1, 2, 3, 5, 8}) {
        std::vector<std::string> pieces;
        std::vector<uint8_t> starts;
        const auto m = make_model(order, rng, words, &pieces, &starts);
        check_probes(*m, rng, (int)words.size() + 3);
        for (int Tp : {1, 12, 40}) {
            check_search(*m, rng, 3, Tp, 1, 1, 0.0, 0.5);
            check_search(*m, rng, 3, Tp, 2, 0, 0.3, 0.5);
            check_search(*m, rng, 3, Tp, 5, 3, 0.25, 2.0);
            check_search(*m, rng, 3, Tp, 32, 8, 0.25, 0.5);
            check_search(*m, rng, 2, Tp, 32, 32 < m->d.vocab - 1 ? 32 : m->d.vocab - 1, 0.0, 0.0);
        }
        // refusals
        CtcNgramArgs a;
        a.d = m->d;
        CHECK(!cg_check(a, false).empty(), "null arguments accepted");
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ctc_ngram_check: all checks held\n");
    return 0;
}
