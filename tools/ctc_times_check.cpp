// Stand-alone host check of the CTC token time stamps: the serial twin the library's host entry runs (csrc/ctc_times_search.h:
// ct_align_host, built from the step functions the kernel is built from) on the CPU, every array a heap block of exactly the size
// the functions were told, so that a sanitizer sees any read or write past a row.  It is held against a naive aligner that shares none
// of the twin's machinery: the whole alpha matrix, one byte per back-pointer, spans collected from the full state sequence.  Spans,
// status, conf and the float64 score must be equal exactly; entries behind a row's labels must keep their sentinels.
// The shapes are those of tests/ctc_times_cases.py (T' 1, 2, 7, 40, 300; V 8 and 5000; batches of 1, 3 and 33; L up to 150; ld > L;
// bad labels; counts out of range; rows on a grid of quarters; rows holding -inf) and random ones.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/ctc_times_check.cpp -o ctc_times_check
// Exit status 0 when every check held.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

#include "ctc_times_search.h"

namespace {

constexpr int32_t SENT_I = -77;
constexpr float SENT_F = -7.5f;

struct Result {
    int status = 0;
    std::vector<int32_t> start, end;
    std::vector<float> conf;
    double score = 0.0;
};

Result naive(const float* lp, int Tp, int V, int n, const int32_t* lab, int L, int blank) {
    const double ninf = -std::numeric_limits<double>::infinity();
    Result r;
    r.start.assign(L, -1), r.end.assign(L, -1), r.conf.assign(L, 0.f);
    r.score = ninf;
    n = std::min(std::max(n, 0), Tp);
    int need = L;
    for (int u = 0; u < L; ++u) {
        if (lab[u] < 0 || lab[u] >= V || lab[u] == blank) r.status = 2;
        if (u && lab[u] == lab[u - 1]) ++need;
    }
    if (r.status == 0 && need > n) r.status = 1;
    if (r.status) return r;
    if (n == 0) {
        r.score = 0.0;
        return r;
    }
    const int S = 2 * L + 1;
    std::vector<int> path(S, blank);
    for (int u = 0; u < L; ++u) path[2 * u + 1] = lab[u];
    std::vector<std::vector<double>> al(n, std::vector<double>(S, ninf));
    std::vector<std::vector<unsigned char>> bp(n, std::vector<unsigned char>(S, 0));
    al[0][0] = lp[path[0]];
    if (S > 1) al[0][1] = lp[path[1]];
    for (int t = 1; t < n; ++t)
        for (int s = 0; s < S; ++s) {
            double best = al[t - 1][s];
            int mv = 0;
            if (s >= 1 && al[t - 1][s - 1] > best) best = al[t - 1][s - 1], mv = 1;
            if (s >= 2 && (s % 2) == 1 && path[s - 2] != path[s] && al[t - 1][s - 2] > best) best = al[t - 1][s - 2], mv = 2;
            al[t][s] = best + (double)lp[(size_t)t * V + path[s]];
            bp[t][s] = (unsigned char)mv;
        }
    int cur = L == 0 ? 0 : (al[n - 1][2 * L - 1] >= al[n - 1][2 * L] ? 2 * L - 1 : 2 * L);
    r.score = al[n - 1][cur];
    std::vector<int> states(n);
    for (int t = n - 1; t >= 0; --t) {
        states[t] = cur;
        cur -= bp[t][cur];
    }
    for (int u = 0; u < L; ++u) {
        float c = 0.f;
        for (int t = 0; t < n; ++t)
            if (states[t] == 2 * u + 1) {
                const float v = lp[(size_t)t * V + lab[u]];
                if (r.start[u] < 0) r.start[u] = t, c = v;
                r.end[u] = t + 1;
                if (v > c) c = v;
            }
        r.conf[u] = c;
    }
    return r;
}

struct Batch {
    int B, Tp, V, ld, blank;
    std::unique_ptr<float[]> logp;
    std::unique_ptr<int32_t[]> frames, labels, label_len;
};

enum Kind { SOFT, GRID, WITH_INF };

Batch make(std::mt19937& rng, int B, int Tp, int V, int ld, int maxL, Kind kind, int blank, bool abuse) {
    Batch x{B, Tp, V, ld, blank, std::make_unique<float[]>((size_t)B * Tp * V), std::make_unique<int32_t[]>(B), std::make_unique<int32_t[]>((size_t)B * ld),
            std::make_unique<int32_t[]>(B)};
    std::uniform_real_distribution<float> uf(-8.f, 0.f);
    std::uniform_int_distribution<int> q(0, 8), pct(0, 99);
    for (size_t i = 0; i < (size_t)B * Tp * V; ++i) {
        x.logp[i] = kind == GRID ? -0.25f * (float)q(rng) : uf(rng);
        if (kind == WITH_INF && pct(rng) < 12) x.logp[i] = -std::numeric_limits<float>::infinity();
    }
    for (int b = 0; b < B; ++b) {
        x.frames[b] = std::uniform_int_distribution<int>(0, Tp)(rng);
        const int L = std::uniform_int_distribution<int>(0, std::min(maxL, ld))(rng);
        x.label_len[b] = L;
        for (int u = 0; u < ld; ++u) {
            int y = std::uniform_int_distribution<int>(0, V - 1)(rng);
            if (y == blank) y = (y + 1) % V;
            if (V > 1 && u && pct(rng) < 30) y = x.labels[(size_t)b * ld + u - 1];  // repeats
            x.labels[(size_t)b * ld + u] = u < L ? y : SENT_I;
        }
        if (abuse) {  // counts out of range, bad labels
            const int what = pct(rng) % 6;
            if (what == 0) x.frames[b] = Tp + 5;
            if (what == 1) x.frames[b] = -3;
            if (what == 2) x.label_len[b] = ld + 4;
            if (what == 3) x.label_len[b] = -2;
            if (what == 4 && L) x.labels[(size_t)b * ld + L / 2] = blank;
            if (what == 5 && L) x.labels[(size_t)b * ld + L - 1] = pct(rng) < 50 ? V : -1;
        }
    }
    return x;
}

long checks = 0;

bool run(const Batch& x, const char* what) {
    const size_t rows = (size_t)x.B * x.ld;
    auto start = std::make_unique<int32_t[]>(rows), end = std::make_unique<int32_t[]>(rows);
    auto conf = std::make_unique<float[]>(rows);
    auto score = std::make_unique<double[]>(x.B);
    auto status = std::make_unique<int32_t[]>(x.B);
    for (size_t i = 0; i < rows; ++i) start[i] = end[i] = SENT_I, conf[i] = SENT_F;
    CtcTimesArgs a;
    a.logp = x.logp.get(), a.frames = x.frames.get(), a.labels = x.labels.get(), a.label_len = x.label_len.get();
    a.B = x.B, a.Tp = x.Tp, a.V = x.V, a.ld = x.ld, a.blank = x.blank;
    a.start = start.get(), a.end = end.get(), a.conf = conf.get(), a.score = score.get(), a.status = status.get();
    const std::string bad = ct_check(a);
    if (!bad.empty()) {
        std::printf("%s: refused: %s\n", what, bad.c_str());
        return false;
    }
    for (int b = 0; b < x.B; ++b) ct_align_host(a, b);
    for (int b = 0; b < x.B; ++b) {
        const int L = std::min(std::max(x.label_len[b], 0), x.ld);
        const Result r = naive(x.logp.get() + (size_t)b * x.Tp * x.V, x.Tp, x.V, x.frames[b], x.labels.get() + (size_t)b * x.ld, L, x.blank);
        bool ok = status[b] == r.status && std::memcmp(&score[b], &r.score, 8) == 0;
        for (int u = 0; u < x.ld; ++u) {
            const size_t i = (size_t)b * x.ld + u;
            if (u < L)
                ok = ok && start[i] == r.start[u] && end[i] == r.end[u] && std::memcmp(&conf[i], &r.conf[u], 4) == 0;
            else
                ok = ok && start[i] == SENT_I && end[i] == SENT_I && conf[i] == SENT_F;
        }
        ++checks;
        if (!ok) {
            std::printf("%s: utterance %d differs (status %d / %d, score %.17g / %.17g)\n", what, b, status[b], r.status, score[b], r.score);
            return false;
        }
    }
    return true;
}

bool refusals() {
    std::mt19937 rng(1);
    Batch x = make(rng, 2, 7, 8, 4, 3, SOFT, 0, false);
    int32_t o[8];
    float c[8];
    double sc[2];
    int32_t st[2];
    CtcTimesArgs a;
    a.logp = x.logp.get(), a.frames = x.frames.get(), a.labels = x.labels.get(), a.label_len = x.label_len.get();
    a.B = 2, a.Tp = 7, a.V = 8, a.ld = 4, a.blank = 0;
    a.start = o, a.end = o, a.conf = c, a.score = sc, a.status = st;
    bool ok = ct_check(a).empty();
    for (int k = 0; k < 12; ++k) {
        CtcTimesArgs w = a;
        if (k == 0) w.logp = nullptr;
        if (k == 1) w.status = nullptr;
        if (k == 2) w.B = 0;
        if (k == 3) w.B = CT_MAX_B + 1;
        if (k == 4) w.Tp = 0;
        if (k == 5) w.Tp = CT_MAX_TP + 1;
        if (k == 6) w.V = 0;
        if (k == 7) w.V = CT_MAX_V + 1;
        if (k == 8) w.ld = 0;
        if (k == 9) w.ld = CT_MAX_LD + 1;
        if (k == 10) w.blank = -1;
        if (k == 11) w.blank = 8;
        ok = ok && !ct_check(w).empty();
    }
    // the launch geometry: the widest rows still fit the scratch form, the threshold switches the form
    ok = ok && ct_lds_fixed(2 * CT_MAX_LD + 1) <= CT_LDS_CAP && ct_bp_in_lds(250, 80, -1) && !ct_bp_in_lds(250, 80, 0) && !ct_bp_in_lds(3000, 42, -1);
    ok = ok && ct_bp_in_lds(7, 9, 7 * 19) && !ct_bp_in_lds(7, 9, 7 * 19 - 1) && ct_scratch_bytes(3, 7, 9, 0) == 3u * 6 * 1 * 16 && ct_scratch_bytes(3, 1, 9, 0) == 0;
    return ok;
}

}  // namespace

int main() {
    std::mt19937 rng(20240607);
    bool ok = refusals();
    if (!ok) std::printf("refusals / geometry: failed\n");
    // the case list's shapes
    const int shapes[][5] = {{3, 1, 8, 3, 1},      {1, 1, 8, 1, 1},      {3, 2, 8, 4, 2},      {9, 7, 8, 9, 7},     {9, 7, 8, 11, 7},
                             {33, 40, 5000, 37, 35}, {7, 300, 8, 153, 150}, {1, 300, 5000, 42, 40}, {3, 40, 5000, 5, 3}, {2, 7, 4, 4, 2}};
    for (const auto& s : shapes)
        for (int kind = 0; kind < 3 && ok; ++kind)
            for (int abuse = 0; abuse < 2 && ok; ++abuse) {
                char what[96];
                std::snprintf(what, sizeof what, "B %d T' %d V %d ld %d kind %d abuse %d", s[0], s[1], s[2], s[3], kind, abuse);
                ok = run(make(rng, s[0], s[1], s[2], s[3], s[4], (Kind)kind, kind == 1 ? 0 : 3 % s[2], abuse != 0), what);
            }
    // random ones: short rows where every tie rule and the feasibility edge are hit often
    for (int i = 0; i < 600 && ok; ++i) {
        const int B = 1 + (int)(rng() % 4), Tp = 1 + (int)(rng() % 12), V = 2 + (int)(rng() % 7), ld = 1 + (int)(rng() % 8);
        char what[96];
        std::snprintf(what, sizeof what, "random %d: B %d T' %d V %d ld %d", i, B, Tp, V, ld);
        ok = run(make(rng, B, Tp, V, ld, ld, (Kind)(i % 3), (int)(rng() % V), i % 4 == 3), what);
    }
    std::printf("%s: %ld utterances checked\n", ok ? "ok" : "FAILED", checks);
    return ok ? 0 : 1;
}
