// Stand-alone host check of the scorer's edit alignment: the serial twin the library's host entry runs (csrc/edit_align_search.h:
// ea_run_host, built from the step functions the kernel is built from) on the CPU, every array a heap block of exactly the size the
// functions were told, so that a sanitizer sees any read or write past a span.  It is held against a naive aligner that shares none of
// the twin's machinery: the whole table, one byte per back-pointer, the plain recurrence with the left neighbour.  Cost, counts, path
// length and paths must be equal exactly; bytes behind a path and rows behind N must keep their sentinels.
// The shapes are those of tests/edit_cases.py (R, H in 0 .. 2; H 62 .. 65 and 127 .. 129; one unit against 300; equal and disjoint
// sequences; runs of one id; 1100 x 900; ids 0, -1, 2^31 - 1; 70 ragged pairs on shared references; clamped lengths; spans that leave
// their buffers; the refusals) and random ones, under the cost triples 1/1/1, 4/3/3 and 1/2/3.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/edit_align_check.cpp -o edit_align_check
// Exit status 0 when every check held.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

#include "edit_align_search.h"

namespace {

constexpr int32_t SENT_I = -77;
constexpr uint8_t SENT_B = 0xEE;
int failures = 0;

void fail(const char* what, const char* name, int n) {
    std::printf("FAIL %s: %s (pair %d)\n", name, what, n);
    ++failures;
}

struct Pair {
    std::vector<int32_t> ref, hyp;
    int ref_len, hyp_len;  // what the caller claims (may differ from the sizes: clamping)
    int share = -1;        // >= 0: this pair uses the reference of that pair
};

struct Naive {
    int cost = 0;
    std::vector<uint8_t> path;
};

Naive naive(const int32_t* ref, int R, const int32_t* hyp, int H, int cs, int ci, int cd) {
    std::vector<std::vector<int>> D(R + 1, std::vector<int>(H + 1, 0));
    std::vector<std::vector<uint8_t>> bp(R + 1, std::vector<uint8_t>(H + 1, 0));
    for (int j = 1; j <= H; ++j) D[0][j] = j * ci, bp[0][j] = 2;
    for (int i = 1; i <= R; ++i) {
        D[i][0] = i * cd, bp[i][0] = 1;
        for (int j = 1; j <= H; ++j) {
            int best = D[i - 1][j - 1] + (ref[i - 1] == hyp[j - 1] ? 0 : cs), b = 0;
            if (D[i - 1][j] + cd < best) best = D[i - 1][j] + cd, b = 1;
            if (D[i][j - 1] + ci < best) best = D[i][j - 1] + ci, b = 2;
            D[i][j] = best, bp[i][j] = (uint8_t)b;
        }
    }
    Naive out;
    out.cost = D[R][H];
    int i = R, j = H;
    while (i || j) {
        const int b = bp[i][j];
        if (b == 0) out.path.push_back(ref[i - 1] == hyp[j - 1] ? 0 : 1), --i, --j;
        else if (b == 1) out.path.push_back(2), --i;
        else out.path.push_back(3), --j;
    }
    std::reverse(out.path.begin(), out.path.end());
    return out;
}

// exact-size heap copies, so that the sanitizer guards both ends of every array
template <class T>
std::unique_ptr<T[]> block(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

void run(const char* name, const std::vector<Pair>& pairs, int max_ref, int max_hyp, int cs, int ci, int cd, int break_span = -1) {
    const int N = (int)pairs.size();
    std::vector<int32_t> ref, hyp, rl, hl;
    std::vector<int64_t> rb(N), hb(N), ob(N);
    int64_t ops_total = 0;
    for (int n = 0; n < N; ++n) {
        const Pair& q = pairs[n];
        if (q.share >= 0)
            rb[n] = rb[q.share];
        else {
            rb[n] = (int64_t)ref.size();
            ref.insert(ref.end(), q.ref.begin(), q.ref.end());
        }
        hb[n] = (int64_t)hyp.size();
        hyp.insert(hyp.end(), q.hyp.begin(), q.hyp.end());
        rl.push_back(q.ref_len), hl.push_back(q.hyp_len);
        ob[n] = ops_total;
        ops_total += ea_clamp(q.ref_len, 0, max_ref) + ea_clamp(q.hyp_len, 0, max_hyp);
    }
    if (break_span >= 0) {  // one pair's spans leave the buffers in turn
        rb[break_span % N] = (int64_t)ref.size() + 1;
        hb[(break_span + 1) % N] = -1;
        ob[(break_span + 2) % N] = ops_total;
    }
    auto ref_b = block(ref), hyp_b = block(hyp), rl_b = block(rl), hl_b = block(hl);
    auto rb_b = block(rb), hb_b = block(hb), ob_b = block(ob);
    std::vector<int32_t> cost(N + 1, SENT_I), counts((size_t)(N + 1) * 4, SENT_I), plen(N + 1, SENT_I);
    std::vector<uint8_t> ops((size_t)ops_total, SENT_B);
    auto cost_b = block(cost), counts_b = block(counts), plen_b = block(plen);
    auto ops_b = block(ops);
    EditArgs a;
    a.ref = ref_b.get(), a.ref_begin = rb_b.get(), a.ref_len = rl_b.get(), a.hyp = hyp_b.get(), a.hyp_begin = hb_b.get(), a.hyp_len = hl_b.get();
    a.ops_begin = ob_b.get(), a.ref_total = (int64_t)ref.size(), a.hyp_total = (int64_t)hyp.size(), a.ops_total = ops_total;
    a.N = N, a.max_ref = max_ref, a.max_hyp = max_hyp, a.c_sub = cs, a.c_ins = ci, a.c_del = cd;
    a.cost = cost_b.get(), a.counts = counts_b.get(), a.path_len = plen_b.get(), a.ops = ops_b.get();
    std::string err;
    if (ea_run_host(a, &err) != 0) {
        fail(err.c_str(), name, -1);
        return;
    }
    std::vector<uint8_t> want((size_t)ops_total, SENT_B);
    for (int n = 0; n < N; ++n) {
        const int R = ea_clamp(rl[n], 0, max_ref), H = ea_clamp(hl[n], 0, max_hyp);
        const bool ok = rb[n] >= 0 && hb[n] >= 0 && ob[n] >= 0 && rb[n] + R <= (int64_t)ref.size() && hb[n] + H <= (int64_t)hyp.size() && ob[n] + R + H <= ops_total;
        Naive w;
        int c4[4] = {0, 0, 0, 0};
        if (ok) {
            w = naive(ref.data() + rb[n], R, hyp.data() + hb[n], H, cs, ci, cd);
            for (uint8_t op : w.path) ++c4[op];
            std::copy(w.path.begin(), w.path.end(), want.begin() + ob[n]);
        } else
            w.cost = -1;
        if (a.cost[n] != w.cost) fail("cost", name, n);
        if (a.path_len[n] != (int)w.path.size()) fail("path_len", name, n);
        if (std::memcmp(a.counts + (size_t)n * 4, c4, sizeof c4) != 0) fail("counts", name, n);
    }
    if (ops_total && std::memcmp(a.ops, want.data(), (size_t)ops_total) != 0) fail("ops bytes or the sentinels behind a path", name, -1);
    if (a.cost[N] != SENT_I || a.path_len[N] != SENT_I || a.counts[(size_t)N * 4] != SENT_I || a.counts[(size_t)N * 4 + 3] != SENT_I) fail("row N written", name, N);
}

std::vector<int32_t> ids(std::mt19937& g, int n, int alphabet) {
    std::vector<int32_t> v(n);
    for (auto& x : v) x = (int32_t)(g() % alphabet);
    return v;
}

Pair pair_of(std::vector<int32_t> r, std::vector<int32_t> h) {
    Pair q;
    q.ref_len = (int)r.size(), q.hyp_len = (int)h.size();
    q.ref = std::move(r), q.hyp = std::move(h);
    return q;
}

void refusals() {
    int32_t one = 0, out4[4];
    int64_t zero = 0;
    uint8_t byte = 0;
    EditArgs ok;
    ok.ref = ok.hyp = ok.ref_len = ok.hyp_len = &one, ok.ref_begin = ok.hyp_begin = ok.ops_begin = &zero;
    ok.cost = ok.path_len = &one, ok.counts = out4, ok.ops = &byte, ok.N = 1;
    std::string err;
    auto refused = [&](EditArgs a, const char* what) {
        if (ea_run_host(a, &err) != -1 || err.find(what) == std::string::npos) fail(what, "refusals", -1);
    };
    EditArgs a = ok;
    a.ref = nullptr, refused(a, "null");
    a = ok, a.ops = nullptr, refused(a, "null");
    a = ok, a.N = 0, refused(a, "N must");
    a = ok, a.N = EA_MAX_N + 1, refused(a, "N must");
    a = ok, a.max_ref = -1, refused(a, "max_ref");
    a = ok, a.max_hyp = EA_MAX_LEN + 1, refused(a, "max_hyp");
    a = ok, a.c_sub = 0, refused(a, "costs");
    a = ok, a.c_ins = 256, refused(a, "costs");
    a = ok, a.c_del = -1, refused(a, "costs");
    a = ok, a.hyp_total = -1, refused(a, "sizes");
    if (ea_run_host(ok, &err) != 0 || one != 0) fail("the plain call", "refusals", -1);
}

}  // namespace

int main() {
    std::mt19937 g(20260);
    const int triples[3][3] = {{1, 1, 1}, {4, 3, 3}, {1, 2, 3}};
    refusals();
    for (const auto& t : triples) {
        const int cs = t[0], ci = t[1], cd = t[2];
        std::vector<Pair> v;
        for (int R = 0; R < 3; ++R)
            for (int H = 0; H < 3; ++H) v.push_back(pair_of(std::vector<int32_t>(R, 5), std::vector<int32_t>(H, 5))), v.push_back(pair_of(ids(g, R, 2), ids(g, H, 2)));
        run("tiny", v, 2, 2, cs, ci, cd);
        run("tiny-slack", v, 9, 7, cs, ci, cd);
        run("tiny-max-zero", v, 0, 0, cs, ci, cd);
        v.clear();
        for (int R : {5, 63, 64, 65})
            for (int H : {62, 63, 64, 65, 127, 128, 129}) v.push_back(pair_of(ids(g, R, 4), ids(g, H, 4)));
        run("widths", v, 65, 129, cs, ci, cd);
        std::vector<int32_t> run300(300, 4);
        for (int at : {0, 150, 299}) {
            std::vector<int32_t> h = run300;
            h[at] = 3;
            run("one-against-300", {pair_of({3}, h), pair_of(h, {3}), pair_of({3}, run300)}, 300, 300, cs, ci, cd);
        }
        const std::vector<int32_t> same = ids(g, 200, 50);
        std::vector<int32_t> other = ids(g, 150, 50);
        for (auto& x : other) x += 100;
        run("equal-disjoint", {pair_of(same, same), pair_of(same, other)}, 200, 200, cs, ci, cd);
        run("runs", {pair_of({7, 7, 7, 7}, {7, 7}), pair_of({7, 7}, {7, 7, 7, 7}), pair_of(std::vector<int32_t>(70, 7), std::vector<int32_t>(66, 7)),
                     pair_of({7, 7, 8, 7, 7}, {7, 7}), pair_of({1, 2, 2, 1}, {2, 1, 1, 2, 2})}, 70, 66, cs, ci, cd);
        run("big", {pair_of(ids(g, 1100, 6), ids(g, 900, 6))}, 1100, 900, cs, ci, cd);
        run("ids", {pair_of({0, -1, INT32_MAX, INT32_MIN, 0}, {-1, 0, INT32_MAX, 0}), pair_of({-1, -1, -1}, {INT32_MAX, INT32_MAX, INT32_MAX})}, 5, 4, cs, ci, cd);
        v.clear();
        for (int n = 0; n < 70; ++n) {
            Pair q = pair_of(n % 7 == 0 ? ids(g, (int)(g() % 41), 8) : std::vector<int32_t>(), ids(g, (int)(g() % 45), 8));
            if (n % 7) q.share = n - n % 7, q.ref_len = v[q.share].ref_len;
            v.push_back(q);
        }
        run("n70-shared", v, 41, 45, cs, ci, cd);
        run("n70-spans", v, 41, 45, cs, ci, cd, 11);
        // claimed lengths above max_* and below 0 are clamped (the arrays hold exactly the clamped counts)
        Pair c1 = pair_of(ids(g, 20, 4), ids(g, 33, 4)), c2 = c1, c3 = c1, c4 = c1;
        c1.ref_len = 50, c1.hyp_len = 60, c2.ref_len = -3, c3.hyp_len = -1, c4.ref_len = c4.hyp_len = INT32_MAX;
        run("clamped", {c1, c2, c3, c4}, 20, 33, cs, ci, cd);
        for (int k = 0; k < 60; ++k) {
            v.clear();
            const int N = 1 + (int)(g() % 5), alphabet = 2 + (int)(g() % 6);
            int mr = 0, mh = 0;
            for (int n = 0; n < N; ++n) {
                v.push_back(pair_of(ids(g, (int)(g() % 150), alphabet), ids(g, (int)(g() % 150), alphabet)));
                mr = std::max(mr, v.back().ref_len), mh = std::max(mh, v.back().hyp_len);
            }
            run("random", v, mr + (int)(g() % 3), mh + (int)(g() % 3), cs, ci, cd);
        }
    }
    std::printf(failures ? "%d checks failed\n" : "edit_align_check: all checks held\n", failures);
    return failures ? 1 : 0;
}
