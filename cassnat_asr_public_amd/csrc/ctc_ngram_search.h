// CTC prefix beam search with word n-gram fusion: score_lm of the shared search (ctc_search.h) formed from an ARPA model - the n-gram
// state of a hypothesis and its update - and the serial host search (cn_ctc_ngram_beam_host; tools/ctc_ngram_check.cpp builds it with
// a plain C++ compiler under sanitizers).  The kernel (ctc_beam.hip) and the host search are made of the same functions.
//
// The contract is in include/cassnat_hip_ctc_ngram.h.  A hypothesis carries the piece-monoid carry of its open
// word, its last NG_HIST word ids (<s> in front), its word count, and - looked up once, when the open word changes - the id of the
// open word and what closing it adds: double(ng_word_score(history, word)) * lm_scale.  A candidate that appends a real piece which
// begins with a separator to a hypothesis with a non-empty open word closes that word and adds the parent's cached value; every
// other candidate adds nothing.  Labels equal to CG_DROP are left out of the gluing, as the ranker does with drop_id = 2.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/cassnat_hip_ctc_ngram.h"
#include "ctc_search.h"

constexpr int CG_DROP = 2;

struct CtcNgramArgs : CtcBeamArgs {  // (out.score_lm is written)
    cn_ngram_desc d;
    double lm_scale = 0.0;  // ctc_lm_weight * ln(10)
};
inline CtcNgramArgs ctc_ngram_args(const cn_ngram_desc& d, double lm_scale, const CtcBeamArgs& search) {
    CtcNgramArgs a;
    static_cast<CtcBeamArgs&>(a) = search;
    a.d = d, a.lm_scale = lm_scale;
    return a;
}
#ifdef __HIPCC__
int launch_ctc_ngram_beam(const CtcNgramArgs& a, hipStream_t s);
#endif

struct CgHyp {
    NgPiece carry;          // the open word
    int32_t hist[NG_HIST];  // the last word ids, oldest first; d.bos in front
    int32_t nwords;         // words closed so far
    int32_t close_wid;      // id of the open word (carry.pw != 1)
    double slm;             // score_lm
    double close_add;       // what closing the open word adds to score_lm
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

// score_lm of the candidate that appends label tok (-1: stay) to the hypothesis with n-gram state h
NG_HD double cg_candidate_slm(const cn_ngram_desc& d, const CgHyp& h, int tok) { return cg_closes(d, h, tok) ? h.slm + h.close_add : h.slm; }

// ---- host only -------------------------------------------------------------------------------------------------------------------
// "" when the arguments can be searched (pointers of the caller's side: not dereferenced here), else what is wrong
inline std::string cg_check(const CtcNgramArgs& a, bool need_scratch) {
    const CtcBeamOut& o = a.out;
    if (!a.logp || !a.size_ratio || (a.P > 0 && !a.top_idx) || !o.hyp || !o.hyp_len || !o.score || !o.score_lm || !o.p_blk || !o.p_nblk ||
        !o.n_out || (need_scratch && (!a.hist_parent || !a.hist_tok)))
        return "null argument";
    if (const char* bad = cs_check_limits(a.W, a.P, 0, 0)) return bad;
    const std::string bad = ng_check_desc(a.d);
    if (!bad.empty()) return bad;
    if (a.B < 1 || a.Tp < 1 || a.V < 1) return "B, T' and V must be positive";
    if (a.blank < 0 || a.blank >= a.V) return "blank must be an id of the vocabulary";
    if (const char* cap = cs_check_limits(a.W, a.P, a.Tp, o.Lmax)) return cap;
    if (!(a.lp == a.lp) || !(a.lm_scale == a.lm_scale)) return "length_penalty and lm_scale must be numbers";
    return "";
}

// double(score of word w behind h's history) * lm_scale, from the probes
inline double cg_word_add(const cn_ngram_desc& d, const CgHyp& h, int32_t w, double lm_scale) {
    NgProbe pr[NG_TASKS];
    const int c = cg_context(d, h);
    for (int t = 0; t < NG_TASKS - 1; ++t) ng_probe(d, h.hist + NG_HIST, c, w, t, &pr[t]);
    return (double)ng_probe_score(pr, c) * lm_scale;
}

// utterance b of `a`, every pointer a host pointer; the back-pointers are kept here, a.hist_parent / a.hist_tok are not used.  The
// order comes from std::stable_sort: the independent check of cs_rank.
inline void cg_search_host(const CtcNgramArgs& a, int b) {
    struct Cand {
        CsCand c;
        double slm, key;
    };
    const cn_ngram_desc& d = a.d;
    const int W = a.W, P = a.P;
    std::vector<CsKept> kept(W);
    std::vector<int> blast(W), order;
    std::vector<CgHyp> hy[2] = {std::vector<CgHyp>(W), std::vector<CgHyp>(W)};
    std::vector<Cand> cand;
    std::vector<unsigned char> hpar((size_t)a.Tp * W);
    std::vector<int> htok((size_t)a.Tp * W);
    const float* logp = a.logp + (long long)b * a.Tp * a.V;
    const int* top = a.top_idx + (long long)b * a.Tp * P;
    const int ssz = cs_src_size(a.size_ratio[b], a.Tp);
    kept[0] = CsKept{0.0, 0.0, 0.0, CS_LOGZERO, 0};  // score_ctc 0, p_blk logone, p_nblk logzero, hyp []
    blast[0] = -1;
    cg_init(d, &hy[0][0]);
    int nb = 1, steps = 0, cur = 0;
    for (int t = 0; t <= ssz && t < a.Tp; ++t) {
        const float* row = logp + (long long)t * a.V;
        if (cs_skip_frame(row[a.blank])) continue;
        cand.clear();
        order.clear();
        for (int k = 0; k < nb; ++k)
            for (int j = 0; j <= P; ++j) {
                const int c = j == 0 ? -1 : top[(long long)t * P + (j - 1)];
                Cand x;
                x.c = cs_candidate(row, a.V, a.blank, k, j == 0, c, kept[k].p_blk, kept[k].p_nblk, blast[k], kept[k].len);
                if (x.c.par < 0) continue;
                x.slm = cg_candidate_slm(d, hy[cur][k], x.c.tok);
                x.key = cs_key(x.c.tot, x.slm, a.lp, x.c.len);
                order.push_back((int)cand.size());
                cand.push_back(x);
            }
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cand[x].key > cand[y].key; });
        const int keep = (int)order.size() < W ? (int)order.size() : W;
        std::vector<CsKept> next(W);
        for (int r = 0; r < keep; ++r) {
            const CsCand& c = cand[order[r]].c;
            next[r] = CsKept{c.tot, 0.0, c.pb, c.pnb, c.len};
            blast[r] = c.last;  // (every parent's state was read into `cand` above)
            hpar[(size_t)steps * W + r] = (unsigned char)c.par;
            htok[(size_t)steps * W + r] = c.tok;
            CgHyp* h = &hy[cur ^ 1][r];
            if (cg_advance(d, hy[cur][c.par], c.tok, h) && h->carry.pw != 1) {
                h->close_wid = ng_word_id(d, h->carry.h);
                h->close_add = cg_word_add(d, *h, h->close_wid, a.lm_scale);
            }
        }
        kept.swap(next);
        nb = keep, ++steps, cur ^= 1;
    }
    // the open word, then </s>; one more stable sort by the same key
    std::vector<double> key(nb);
    order.clear();
    for (int r = 0; r < nb; ++r) {
        CgHyp& h = hy[cur][r];
        if (h.carry.pw != 1) cg_push_word(&h, h.close_wid, h.close_add);
        h.slm += cg_word_add(d, h, d.eos, a.lm_scale);
        kept[r].score_lm = h.slm;
        key[r] = cs_key(kept[r].score, h.slm, a.lp, kept[r].len);
        order.push_back(r);
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] > key[y]; });
    a.out.n_out[b] = nb;
    for (int r = 0; r < W; ++r)
        cs_write_row(a.out, (long long)b * W + r, hpar.data(), htok.data(), 0, W, steps, r < nb ? order[r] : -1, kept[r < nb ? order[r] : 0]);
}
