// CTC prefix beam search with word n-gram fusion: the step functions the kernel (ctc_ngram.hip) and the serial host search are both
// made of - candidate arithmetic, the n-gram state of a hypothesis and its update, the word score as independent table probes - and
// the host search itself (cn_ctc_ngram_beam_host; tools/ctc_ngram_check.cpp builds it with a plain C++ compiler under sanitizers).
//
// The search is ctc_beam_decode's (ctc_beam.hip) in everything but score_lm (contract: include/cassnat_hip_ctc_ngram.h).  A hypothesis carries the piece-monoid carry of its open
// word, its last NG_HIST word ids (<s> in front), its word count, and - looked up once, when the open word changes - the id of the
// open word and what closing it adds: double(ng_word_score(history, word)) * lm_scale.  A candidate that appends a real piece which
// begins with a separator to a hypothesis with a non-empty open word closes that word and adds the parent's cached value; every
// other candidate adds nothing.  Labels equal to CG_DROP are left out of the gluing, as the ranker does with drop_id = 2.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/cassnat_hip_ctc_ngram.h"
#include "ngram_core.h"

#define CG_LOGZERO (-1e10)
constexpr int CG_DROP = 2;
constexpr int CG_MAX_BEAM = 32, CG_MAX_PRUNE = 32;
constexpr int CG_TASKS = 2 * NG_MAX_ORDER;  // probes of one word: NG_MAX_ORDER k-grams, NG_MAX_ORDER - 1 back-off weights, one idle

struct CtcNgramArgs {
    cn_ngram_desc d;
    const float* logp = nullptr;        // [B][Tp][V] CTC log-posteriors of ALL frames
    const int* top_idx = nullptr;       // [B][Tp][P] pruned labels per frame, in list order (may be null when P = 0)
    const float* size_ratio = nullptr;  // [B]
    int B = 0, Tp = 0, V = 0, P = 0, W = 0, blank = 0, Lmax = 0;
    double lp = 0.0;        // args.ctc_lp
    double lm_scale = 0.0;  // ctc_lm_weight * ln(10)
    unsigned char* hist_parent = nullptr;  // [B][Tp][W] scratch
    int* hist_tok = nullptr;               // [B][Tp][W] scratch
    int* hyp = nullptr;           // [B][W][Lmax]
    int* hyp_len = nullptr;       // [B][W]
    double* score = nullptr;      // [B][W] score_ctc
    double* score_lm = nullptr;   // [B][W]
    double* p_blk = nullptr;      // [B][W]
    double* p_nblk = nullptr;
    int* n_out = nullptr;         // [B] hypotheses kept
};
#ifdef __HIPCC__
int launch_ctc_ngram_beam(const CtcNgramArgs& a, hipStream_t s);
#endif

NG_HD double cg_logaddexp(double x, double y) {  // numpy's npy_logaddexp
    if (x == y) return x + 0.693147180559945309417232121458176568;
    const double tmp = x - y;
    if (tmp > 0) return x + log1p(exp(-tmp));
    if (tmp <= 0) return y + log1p(exp(tmp));
    return tmp;
}

// src_size = (ratio * T').long(): fp32 product, truncation (beam_decode.py:22); frames t <= src_size are looked at, so everything
// from T' - 1 up means "all" and everything below 0 "none" (a ratio that is no number: none)
NG_HD int cg_src_size(float ratio, int Tp) {
    const float r = ratio * (float)Tp;
    return r >= (float)Tp ? Tp : (r > -1.f ? (int)r : -1);
}

// a frame is skipped when torch.exp of its float32 blank log-posterior exceeds the double 0.95
NG_HD bool cg_skip_frame(float pblank) { return (double)(float)exp((double)pblank) > 0.95; }

struct CgHyp {
    NgPiece carry;          // the open word
    int32_t hist[NG_HIST];  // the last word ids, oldest first; d.bos in front
    int32_t nwords;         // words closed so far
    int32_t close_wid;      // id of the open word (carry.pw != 1)
    double slm;             // score_lm
    double close_add;       // what closing the open word adds to score_lm
};

struct CgCand {
    double pb, pnb, tot, slm, key;
    int par, tok, len, last;  // par -1: not a candidate; tok -1: stay
};

struct NgProbe {
    float prob, bo;
    int found;
};

NG_HD void cg_init(const cn_ngram_desc& d, CgHyp* h) {
    h->carry = ng_piece(d, 0, false);
    for (int i = 0; i < NG_HIST; ++i) h->hist[i] = d.bos;
    h->nwords = 0;
    h->close_wid = -1;
    h->slm = 0.0;
    h->close_add = 0.0;
}

// length of the history a word after h's words is scored with
NG_HD int cg_context(const cn_ngram_desc& d, const CgHyp& h) { return h.nwords + 1 < d.order - 1 ? h.nwords + 1 : d.order - 1; }

NG_HD bool cg_closes(const cn_ngram_desc& d, const CgHyp& h, int tok) {
    return tok >= 0 && tok != CG_DROP && ng_piece(d, tok, true).starts && h.carry.pw != 1;
}

NG_HD void cg_push_word(CgHyp* h, int32_t w, double add) {
    h->slm += add;
    for (int i = 0; i + 1 < NG_HIST; ++i) h->hist[i] = h->hist[i + 1];
    h->hist[NG_HIST - 1] = w;
    ++h->nwords;
}

// the state of `parent` with `tok` appended (-1: stay); true when the open word changed: then close_wid / close_add of *out are to be
// looked up if out->carry.pw != 1
NG_HD bool cg_advance(const cn_ngram_desc& d, const CgHyp& parent, int tok, CgHyp* out) {
    *out = parent;
    if (tok < 0 || tok == CG_DROP) return false;
    const NgPiece pc = ng_piece(d, tok, true);
    if (pc.starts && parent.carry.pw != 1) cg_push_word(out, parent.close_wid, parent.close_add);
    out->carry = ng_combine(parent.carry, pc);
    out->close_wid = -1;
    out->close_add = 0.0;
    return true;
}

// candidate of hypothesis k (p_b, p_nb, last label or -1, length, n-gram state h): `stay` is blank or a repetition of the last
// label, else label c is appended (blank or an id outside [0, V): no candidate).  row: the frame's V log-posteriors.
NG_HD CgCand cg_candidate(const cn_ngram_desc& d, const float* row, int V, int blank, int k, bool stay, int c, double p_b, double p_nb,
                          int last, int len, const CgHyp& h, double lp) {
    CgCand r;
    r.par = -1, r.tok = -1, r.len = 0, r.last = -1;
    r.pb = r.pnb = r.tot = r.key = CG_LOGZERO;
    r.slm = 0.0;
    if (stay) {
        r.pnb = len > 0 ? p_nb + (double)row[last] : CG_LOGZERO;
        const double pt = (double)row[blank];
        r.pb = cg_logaddexp(p_b + pt, p_nb + pt);
        r.tot = cg_logaddexp(r.pb, r.pnb);
        r.slm = h.slm;
        r.par = k, r.len = len, r.last = last;
    } else if (c >= 0 && c != blank && c < V) {
        const double pt = (double)row[c];
        r.pnb = (c != last) ? cg_logaddexp(p_b + pt, p_nb + pt) : p_b + pt;
        r.pb = CG_LOGZERO;
        r.tot = cg_logaddexp(r.pb, r.pnb);
        r.slm = cg_closes(d, h, c) ? h.slm + h.close_add : h.slm;
        r.par = k, r.tok = c, r.len = len + 1, r.last = c;
    } else {
        return r;
    }
    r.key = (r.tot + r.slm) + lp * (double)r.len;  // score_ctc + score_lm + ctc_lp * len(hyp)
    return r;
}

// The table probes of ng_word_score(d, h, c, w), one per task, independent of each other: task i < NG_MAX_ORDER is the (i + 1)-gram
// that ends in w (needs i <= c), task NG_MAX_ORDER + j - 1 the back-off weight of the j-gram h[-j .. -1] (1 <= j <= c).
NG_HD void cg_probe(const cn_ngram_desc& d, const int32_t* h, int c, int32_t w, int task, NgProbe* out) {
    out->prob = 0.f, out->bo = 0.f, out->found = 0;
    const bool gram = task < NG_MAX_ORDER;
    const int n = gram ? task : task - NG_MAX_ORDER + 1;  // history ids folded
    if (n > c || (!gram && n < 1) || n >= NG_MAX_ORDER) return;
    uint64_t f = gram ? ng_fold(NG_SEED, w) : NG_SEED;
    for (int i = 1; i <= n; ++i) f = ng_fold(f, h[-i]);
    out->found = ng_gram(d, ng_gram_key(f, gram ? n + 1 : n, d.key_mask), &out->prob, &out->bo) ? 1 : 0;
}

// ng_word_score's float32 sum from the probes: the longest k-gram's probability, then the back-off weights for j = k .. c
NG_HD float cg_word_score(const NgProbe* pr, int c) {
    int k = 0;
    float s = NG_UNK_LOGPROB;
    for (int i = NG_MAX_ORDER; i >= 1; --i) {
        if (k == 0 && i <= c + 1 && pr[i - 1].found) k = i, s = pr[i - 1].prob;
    }
    if (k == 0) k = 1;
    for (int j = 1; j < NG_MAX_ORDER; ++j) {
        if (j <= c && j >= k && pr[NG_MAX_ORDER + j - 1].found) s += pr[NG_MAX_ORDER + j - 1].bo;
    }
    return s;
}

// ---- host only -------------------------------------------------------------------------------------------------------------------
// "" when the arguments can be searched (pointers of the caller's side: not dereferenced here), else what is wrong
inline std::string cg_check(const CtcNgramArgs& a, bool need_scratch) {
    const cn_ngram_desc& d = a.d;
    if (!a.logp || !a.size_ratio || (a.P > 0 && !a.top_idx) || !a.hyp || !a.hyp_len || !a.score || !a.score_lm || !a.p_blk || !a.p_nblk ||
        !a.n_out || (need_scratch && (!a.hist_parent || !a.hist_tok)))
        return "null argument";
    if (!d.word_keys || !d.word_ids || !d.gram_keys || !d.gram_prob || !d.gram_bo || !d.piece_hash || !d.piece_pow || !d.piece_starts)
        return "null table in the desc";
    if (a.W < 1 || a.W > CG_MAX_BEAM || a.P < 0 || a.P > CG_MAX_PRUNE) return "need 1 <= ctc_beam <= 32 and 0 <= ctc_pruning <= 32";
    if (d.order < 1 || d.order > NG_MAX_ORDER) return "order " + std::to_string(d.order) + " is outside 1 .. 8";
    if (d.word_slots < 1 || (d.word_slots & (d.word_slots - 1)) || d.gram_slots < 1 || (d.gram_slots & (d.gram_slots - 1)))
        return "the slot counts must be powers of two";
    if (a.B < 1 || a.Tp < 1 || a.V < 1 || d.vocab < 0) return "B, T' and V must be positive, vocab not negative";
    if (a.blank < 0 || a.blank >= a.V) return "blank must be an id of the vocabulary";
    if (a.Lmax < a.Tp + 1) return "hyp_cap must be at least T' + 1";
    if (!(a.lp == a.lp) || !(a.lm_scale == a.lm_scale)) return "length_penalty and lm_scale must be numbers";
    return "";
}

// close_wid / close_add of a hypothesis whose open word changed
inline void cg_lookup_close(const cn_ngram_desc& d, CgHyp* h, double lm_scale) {
    if (h->carry.pw == 1) return;
    h->close_wid = ng_word_id(d, h->carry.h);
    NgProbe pr[CG_TASKS];
    const int c = cg_context(d, *h);
    for (int t = 0; t < CG_TASKS - 1; ++t) cg_probe(d, h->hist + NG_HIST, c, h->close_wid, t, &pr[t]);
    h->close_add = (double)cg_word_score(pr, c) * lm_scale;
}

// utterance b of `a`, every pointer a host pointer; hist_parent / hist_tok are not used
inline void cg_search_host(const CtcNgramArgs& a, int b) {
    const cn_ngram_desc& d = a.d;
    const int W = a.W, P = a.P;
    std::vector<double> pb(W), pnb(W), ptot(W);
    std::vector<int> blen(W), blast(W), order;
    std::vector<CgHyp> hy[2] = {std::vector<CgHyp>(W), std::vector<CgHyp>(W)};
    std::vector<CgCand> cand;
    std::vector<unsigned char> hpar((size_t)a.Tp * W);
    std::vector<int> htok((size_t)a.Tp * W);
    const float* logp = a.logp + (long long)b * a.Tp * a.V;
    const int* top = a.top_idx + (long long)b * a.Tp * P;
    const int ssz = cg_src_size(a.size_ratio[b], a.Tp);
    pb[0] = 0.0, pnb[0] = CG_LOGZERO, ptot[0] = 0.0, blen[0] = 0, blast[0] = -1;
    cg_init(d, &hy[0][0]);
    int nb = 1, steps = 0, cur = 0;
    for (int t = 0; t < a.Tp; ++t) {
        if (t > ssz) continue;  // (the reference does process frame t == src_size)
        const float* row = logp + (long long)t * a.V;
        if (cg_skip_frame(row[a.blank])) continue;
        cand.clear();
        for (int k = 0; k < nb; ++k)
            for (int j = 0; j <= P; ++j) {
                const int c = j == 0 ? -1 : top[(long long)t * P + (j - 1)];
                cand.push_back(cg_candidate(d, row, a.V, a.blank, k, j == 0, c, pb[k], pnb[k], blast[k], blen[k], hy[cur][k], a.lp));
            }
        order.clear();
        for (int i = 0; i < (int)cand.size(); ++i)
            if (cand[i].par >= 0) order.push_back(i);
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cand[x].key > cand[y].key; });
        const int keep = (int)order.size() < W ? (int)order.size() : W;
        for (int r = 0; r < keep; ++r) {
            const CgCand& c = cand[order[r]];
            pb[r] = c.pb, pnb[r] = c.pnb, ptot[r] = c.tot, blen[r] = c.len, blast[r] = c.last;
            hpar[(size_t)steps * W + r] = (unsigned char)c.par;
            htok[(size_t)steps * W + r] = c.tok;
            if (cg_advance(d, hy[cur][c.par], c.tok, &hy[cur ^ 1][r])) cg_lookup_close(d, &hy[cur ^ 1][r], a.lm_scale);
        }
        nb = keep, ++steps, cur ^= 1;
    }
    // the open word, then </s>; one more stable sort by the same key
    std::vector<double> key(nb);
    order.clear();
    for (int r = 0; r < nb; ++r) {
        CgHyp& h = hy[cur][r];
        if (h.carry.pw != 1) cg_push_word(&h, h.close_wid, h.close_add);
        NgProbe pr[CG_TASKS];
        const int c = cg_context(d, h);
        for (int t = 0; t < CG_TASKS - 1; ++t) cg_probe(d, h.hist + NG_HIST, c, d.eos, t, &pr[t]);
        h.slm += (double)cg_word_score(pr, c) * a.lm_scale;
        key[r] = (ptot[r] + h.slm) + a.lp * (double)blen[r];
        order.push_back(r);
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] > key[y]; });
    a.n_out[b] = nb;
    for (int r = 0; r < W; ++r) {
        int* h = a.hyp + ((long long)b * W + r) * a.Lmax;
        const long long o = (long long)b * W + r;
        for (int i = 0; i < a.Lmax; ++i) h[i] = 0;
        if (r >= nb) {
            a.hyp_len[o] = 0;
            a.score[o] = a.p_blk[o] = a.p_nblk[o] = CG_LOGZERO;
            a.score_lm[o] = 0.0;
            continue;
        }
        const int src = order[r], len = blen[src];
        int pos = len - 1, at = src;
        for (int st = steps - 1; st >= 0; --st) {
            const int tok = htok[(size_t)st * W + at];
            if (tok >= 0) {
                if (pos >= 0 && pos < a.Lmax) h[pos] = tok;
                --pos;
            }
            at = hpar[(size_t)st * W + at];
        }
        a.hyp_len[o] = len;
        a.score[o] = ptot[src], a.score_lm[o] = hy[cur][src].slm, a.p_blk[o] = pb[src], a.p_nblk[o] = pnb[src];
    }
}
