// CASS-NAT finish loop with word n-gram fusion: the step functions the kernels (nat_ngram.hip) and the serial host entry
// (cn_nat_ngram_finish_host; tools/nat_ngram_check.cpp builds it with a plain C++ compiler under sanitizers) are both made of.
// The contract is in include/cassnat_hip_nat_ngram.h.
//
// A candidate's term depends on its class alone (eos, a piece that begins a word, any other), and row (b, i) of a non-autoregressive
// pass is the same for every beam slot of utterance b.  So the vocabulary is ranked once per row, per class, by (att descending,
// index ascending) - the class tables - and a slot's beam_width best candidates under its own adds are a three-way merge of the two
// tables' heads and the eos entry: within a class fl32(att + fl32(scale * term)) is monotone in att.  The state that follows a beam
// slot is the AnState of ast_ngram_search.h, advanced by the slot's newest token with the serial walk (an_advance), and a double score.
#pragma once
#include <cmath>
#include <vector>

#include "../../include/cassnat_hip_nat_ngram.h"
#include "ast_ngram_search.h"

constexpr int NN_MAXW = 16, NN_MAXC = NN_MAXW * NN_MAXW;  // beam slots of an utterance, candidates of a step
constexpr int NN_MAXV = 8192;                             // a row sits in LDS

// a value the compiler must take as it is: what is computed from it is not contracted with what computed it
NG_HD float nn_opaque(float p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__ volatile("" : "+v"(p));
#else
    __asm__ volatile("" : "+m"(p));
#endif
    return p;
}
NG_HD double nn_opaque(double p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__ volatile("" : "+v"(p));
#else
    __asm__ volatile("" : "+m"(p));
#endif
    return p;
}

// fl32(att + fl32(scale * term))
NG_HD float nn_fuse(float att, float scale, float term) { return att + nn_opaque(scale * term); }

// score + (len - 1) * length_penalty for the candidates of `step` (step + 2 tokens each), or the score alone
NG_HD double nn_key(double score, int step, int use_lp, double lp) { return use_lp ? score + nn_opaque((double)(step + 1) * lp) : score; }

// 0: any other piece, 1: a piece that begins a word, 2: eos
NG_HD int nn_class(const unsigned char* starts, int32_t eos, int32_t c) { return c == eos ? 2 : (starts[c] ? 1 : 0); }

// candidate order within a slot: fused descending, then att descending, then index ascending
NG_HD bool nn_before(float fa, float aa, int32_t ia, float fb, float ab, int32_t ib) {
    if (fa != fb) return fa > fb;
    if (aa != ab) return aa > ab;
    return ia < ib;
}

// the slot's newest token joins its state; hist[NG_HIST] becomes the id of the open word, which an_probe reads
NG_HD void nn_advance(const cn_ngram_desc& d, AnState* s, bool has_tok, int32_t tok, int32_t eos) {
    if (has_tok) an_advance(d, s, tok, eos);
    s->hist[NG_HIST] = s->carry.pw != 1 ? ng_word_id(d, s->carry.h) : d.bos;
    s->hist[NG_HIST + 1] = d.bos;
}

// The k best candidates of one slot from the class tables of its row (idx / val [2][k]: class 0 then class 1, each best first, padded
// with index -1) and the row's eos entry, under the slot's adds: tok / val [k], best first.  A slot with fewer than k candidates is
// filled up with token 0 at -inf.
NG_HD void nn_merge(const int32_t* idx, const float* val, float eos_val, int32_t eos, const float* adds, float scale, int k, int32_t* tok,
                    float* out) {
    int p0 = 0, p1 = 0;
    bool eos_left = eos_val == eos_val;  // (a NaN is no candidate)
    for (int r = 0; r < k; ++r) {
        int pick = -1;
        float bf = 0.f, ba = 0.f;
        int32_t bi = 0;
        if (p0 < k && idx[p0] >= 0) {
            pick = 0, ba = val[p0], bi = idx[p0], bf = nn_fuse(ba, scale, 0.f);
        }
        if (p1 < k && idx[k + p1] >= 0) {
            const float a = val[k + p1], f = nn_fuse(a, scale, adds[0]);
            if (pick < 0 || nn_before(f, a, idx[k + p1], bf, ba, bi)) pick = 1, ba = a, bi = idx[k + p1], bf = f;
        }
        if (eos_left) {
            const float f = nn_fuse(eos_val, scale, adds[1]);
            if (pick < 0 || nn_before(f, eos_val, eos, bf, ba, bi)) pick = 2, ba = eos_val, bi = eos, bf = f;
        }
        if (pick < 0) {
            tok[r] = 0, out[r] = -INFINITY;
            continue;
        }
        tok[r] = bi, out[r] = bf;
        if (pick == 0) ++p0;
        else if (pick == 1) ++p1;
        else eos_left = false;
    }
}

// The stable descending order as a count (nat_beam_update_kernel's): how many of the n candidates sort before candidate i
NG_HD int nn_rank(const double* key, int n, int i) {
    const double k = key[i];
    int r = 0;
    for (int e = 0; e < n; ++e) r += (key[e] > k) || (key[e] == k && e < i);
    return r;
}

NG_HD int nn_clamp_last(int last, int U, int L) {
    const int cap = U - 1 < L - 2 ? U - 1 : L - 2;
    return last < -1 ? -1 : (last > cap ? cap : last);
}

// ---- host only -------------------------------------------------------------------------------------------------------------------
// "" when the geometry can be searched, else what is wrong
inline std::string nn_check(int B, int U, int V, int bw, int eos, int L) {
    if (B < 1 || U < 1 || V < 1) return "B, U and V must be positive";
    if (V > NN_MAXV) return "the vocabulary must not exceed 8192 entries (a row sits in LDS)";
    if (bw < 1 || bw > NN_MAXW || bw > V) return "need 1 <= beam_width <= min(16, V)";
    if (eos < 0 || eos >= V) return "eos must be an id of the vocabulary";
    if (L < 1) return "max_len must be positive";
    return "";
}

// class tables of one full row (row == nullptr: the all-zero row): one pass, every entry inserted behind the entries that are not
// worse - the serial counterpart of nat_class_topk_kernel's selection rounds
inline void nn_class_topk_row_host(const float* row, int V, const unsigned char* starts, int32_t eos, int k, int32_t* idx, float* val,
                                   float* eos_val) {
    int n[2] = {0, 0};
    for (int j = 0; j < 2 * k; ++j) idx[j] = -1, val[j] = -INFINITY;
    *eos_val = row ? row[eos] : 0.f;
    for (int c = 0; c < V; ++c) {
        const float v = row ? row[c] : 0.f;
        const int cls = nn_class(starts, eos, c);
        if (cls == 2 || v != v) continue;
        int32_t* ci = idx + cls * k;
        float* cv = val + cls * k;
        int p = n[cls];
        while (p > 0 && cv[p - 1] < v) --p;  // (equal values stay in front: the lower index)
        if (p >= k) continue;
        const int end = n[cls] < k ? n[cls] : k - 1;
        for (int j = end; j > p; --j) ci[j] = ci[j - 1], cv[j] = cv[j - 1];
        ci[p] = c, cv[p] = v;
        if (n[cls] < k) ++n[cls];
    }
}

struct NnHostArgs {
    cn_ngram_desc d;
    float scale;
    const float* att;     // [B][U][V]
    const int32_t* ylen;  // [B]
    const int32_t* zlen;  // [B] or null
    int B, U, V, ymax, bw, eos, sos, pad, use_lp, L;
    double lp;
    int32_t* hyp;      // [B][bw][L]
    int32_t* hyp_len;  // [B][bw]
    double* score;     // [B][bw]
};

// utterance b, every pointer a host pointer
inline void nn_search_host(const NnHostArgs& a, int b) {
    const cn_ngram_desc& d = a.d;
    const int bw = a.bw, k = a.bw, U = a.U, V = a.V;
    const int want = a.ylen[b] < a.ymax - 1 ? a.ylen[b] : a.ymax - 1;
    const int last = nn_clamp_last(want, U, a.L);
    std::vector<AnState> st[2] = {std::vector<AnState>(bw), std::vector<AnState>(bw)};
    std::vector<double> sc[2] = {std::vector<double>(bw, 0.0), std::vector<double>(bw, 0.0)};
    std::vector<int32_t> newest[2] = {std::vector<int32_t>(bw, 0), std::vector<int32_t>(bw, 0)};
    std::vector<int32_t> cidx(2 * k), ctok(bw * bw), hist((size_t)(last + 1) * bw * 2);
    std::vector<float> cval(2 * k), fval(bw * bw);
    std::vector<double> ckey(bw * bw), cscore(bw * bw);
    an_init(d, &st[0][0]);
    int cur = 0;
    for (int step = 0; step <= last; ++step) {
        const bool zero = a.zlen && step >= a.zlen[b];
        float eos_val;
        nn_class_topk_row_host(zero ? nullptr : a.att + ((long long)b * U + step) * V, V, d.piece_starts, a.eos, k, cidx.data(), cval.data(),
                               &eos_val);
        const int nl = step == 0 ? 1 : bw, ncand = nl * bw, nxt = cur ^ 1;
        for (int s = 0; s < nl; ++s) {
            nn_advance(d, &st[cur][s], step > 0, newest[cur][s], a.eos);
            NgProbe pr[2 * NG_TASKS];
            float adds[2];
            for (int t = 0; t < 2 * NG_TASKS; ++t) an_probe(d, st[cur][s], t, &pr[t]);
            an_adds(d, st[cur][s], pr, adds);
            nn_merge(cidx.data(), cval.data(), eos_val, a.eos, adds, a.scale, k, &ctok[s * bw], &fval[s * bw]);
        }
        for (int e = 0; e < ncand; ++e) {
            cscore[e] = sc[cur][e / bw] + (double)fval[e];
            ckey[e] = nn_key(cscore[e], step, a.use_lp, a.lp);
        }
        std::vector<int> newslot(bw, 0);  // (NaN keys rank nowhere: every slot still names a candidate)
        for (int e = 0; e < ncand; ++e) {
            const int r = nn_rank(ckey.data(), ncand, e);
            if (r < bw) newslot[r] = e;
        }
        for (int q = 0; q < bw; ++q) {
            const int e = newslot[q], parent = e / bw;
            st[nxt][q] = st[cur][parent];
            sc[nxt][q] = cscore[e];
            newest[nxt][q] = ctok[e];
            hist[((size_t)step * bw + q) * 2] = ctok[e];
            hist[((size_t)step * bw + q) * 2 + 1] = parent;
        }
        cur = nxt;
    }
    for (int j = 0; j < bw; ++j) {
        int32_t* h = a.hyp + ((long long)b * bw + j) * a.L;
        h[0] = a.sos;
        for (int t = last + 2; t < a.L; ++t) h[t] = a.pad;
        int slot = j;
        for (int i = last; i >= 0; --i) {
            h[i + 1] = hist[((size_t)i * bw + slot) * 2];
            slot = hist[((size_t)i * bw + slot) * 2 + 1];
        }
        a.hyp_len[b * bw + j] = last + 2;
        a.score[b * bw + j] = sc[cur][j];
    }
}
