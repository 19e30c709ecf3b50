// CTC prefix beam search, what every policy shares on the host: the one check of a CtcSearchArgs (ctc_search.h) and the one serial
// search, made of the functions the kernel (ctc_beam.hip) is made of - ctc_search.h's, and the state functions of the fusion policies
// (ctc_ngram_search.h, ctc_bias_search.h) and of merging by prefix (ctc_merge_search.h).  A plain C++ compiler reads it:
// tools/ctc_ngram_check.cpp, tools/ctc_bias_check.cpp and tools/ctc_merge_check.cpp build it under sanitizers.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "ctc_merge_search.h"

// "" when the arguments can be searched (pointers of the caller's side: not dereferenced here), else what is wrong
inline std::string ctc_search_check(const CtcSearchArgs& a, bool need_scratch) {
    const CtcBeamOut& o = a.out;
    if (a.ng && a.bias) return "at most one of the n-gram and the bias descriptor may be set";
    if (!a.logp || !a.size_ratio || (a.P > 0 && !a.top_idx) || !o.hyp || !o.hyp_len || !o.score || !o.p_blk || !o.p_nblk || !o.n_out ||
        ((a.ng || a.bias || a.merge) && !o.score_lm) || (need_scratch && (!a.hist_parent || !a.hist_tok)))
        return "null argument";
    if (const char* bad = cs_check_limits(a.W, a.P, 0, 0)) return bad;
    const std::string bad = a.ng ? ng_check_desc(*a.ng) : a.bias ? cb_check_desc(*a.bias) : std::string();
    if (!bad.empty()) return bad;
    if (a.B < 1 || a.Tp < 1 || a.V < 1) return "B, T' and V must be positive";
    if (a.blank < 0 || a.blank >= a.V) return "blank must be an id of the vocabulary";
    if (const char* cap = cs_check_limits(a.W, a.P, a.Tp, o.Lmax)) return cap;
    if (a.ng && !(a.lp == a.lp && a.lm_scale == a.lm_scale)) return "length_penalty and lm_scale must be numbers";
    if (!(a.lp == a.lp)) return "length_penalty must be a number";
    return "";
}

// utterance b of `a`, every pointer a host pointer; the back-pointers are kept here, a.hist_parent / a.hist_tok are not used.  The
// order comes from std::stable_sort and identity from the label vectors: the independent check of cs_rank and of the kernel's
// identity test.
inline void ctc_search_host(const CtcSearchArgs& a, int b) {
    struct Cand {
        CsCand c;
        CbState st;
        double slm, key;
        bool live;
    };
    const int W = a.W, P = a.P;
    std::vector<CsKept> kept(W);
    std::vector<int> blast(W), order, lab(P), stay_at(W);
    std::vector<std::vector<int>> seq(W), nseq(W);
    std::vector<CgHyp> hy[2] = {std::vector<CgHyp>(W), std::vector<CgHyp>(W)};
    std::vector<CbState> st[2] = {std::vector<CbState>(W), std::vector<CbState>(W)};
    std::vector<Cand> cand;
    std::vector<unsigned char> hpar((size_t)a.Tp * W);
    std::vector<int> htok((size_t)a.Tp * W);
    const float* logp = a.logp + (long long)b * a.Tp * a.V;
    const int* top = a.top_idx + (long long)b * a.Tp * P;
    const int ssz = cs_src_size(a.size_ratio[b], a.Tp);
    kept[0] = CsKept{0.0, 0.0, 0.0, CS_LOGZERO, 0};  // score_ctc 0, p_blk logone, p_nblk logzero, hyp []
    blast[0] = -1;
    if (a.ng) cg_init(*a.ng, &hy[0][0]);
    st[0][0] = cb_init();
    int nb = 1, steps = 0, cur = 0;
    for (int t = 0; t <= ssz && t < a.Tp; ++t) {
        const float* row = logp + (long long)t * a.V;
        if (cs_skip_frame(row[a.blank])) continue;
        for (int j = 1; j <= P; ++j) {
            const int c = top[(long long)t * P + (j - 1)];
            lab[j - 1] = a.merge ? cm_dedup(top + (long long)t * P, j, c) : c;
        }
        cand.clear();
        order.clear();
        for (int k = 0; k < nb; ++k)
            for (int j = 0; j <= P; ++j) {
                Cand x;
                x.c = cs_candidate(row, a.V, a.blank, k, j == 0, j == 0 ? -1 : lab[j - 1], kept[k].p_blk, kept[k].p_nblk, blast[k], kept[k].len);
                if (x.c.par < 0) continue;
                x.st = cb_init(), x.slm = 0.0, x.live = true;
                if (a.ng) x.slm = cg_candidate_slm(*a.ng, hy[cur][k], x.c.tok);
                if (a.bias) {
                    x.st = cb_step(*a.bias, st[cur][k], x.c.tok);
                    x.slm = cb_slm(*a.bias, x.st);
                }
                if (j == 0) stay_at[k] = (int)cand.size();
                cand.push_back(x);
            }
        // the fold: an extension that spells a kept hypothesis' labels goes into that hypothesis' stay candidate
        for (Cand& x : cand) {
            if (!a.merge || x.c.tok < 0) continue;
            std::vector<int> s = seq[x.c.par];
            s.push_back(x.c.tok);
            for (int kp = 0; kp < nb; ++kp)
                if (seq[kp] == s) {
                    CsCand& stay = cand[stay_at[kp]].c;
                    cm_fold(stay.pb, &stay.pnb, &stay.tot, x.c.pnb);
                    x.live = false;
                    break;
                }
        }
        for (size_t i = 0; i < cand.size(); ++i)
            if (cand[i].live) {
                cand[i].key = cs_key(cand[i].c.tot, cand[i].slm, a.lp, cand[i].c.len);
                order.push_back((int)i);
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
            nseq[r] = seq[c.par];
            if (c.tok >= 0) nseq[r].push_back(c.tok);
            st[cur ^ 1][r] = cand[order[r]].st;
            if (a.ng) {
                CgHyp* h = &hy[cur ^ 1][r];
                if (cg_advance(*a.ng, hy[cur][c.par], c.tok, h) && h->carry.pw != 1) {
                    h->close_wid = ng_word_id(*a.ng, h->carry.h);
                    h->close_add = cg_word_add(*a.ng, *h, h->close_wid, a.lm_scale);
                }
            }
        }
        kept.swap(next);
        seq.swap(nseq);
        nb = keep, ++steps, cur ^= 1;
    }
    // n-gram: the open word, then </s>; bias: the open match is given up; with either, one more stable sort by the same key
    std::vector<double> key(nb);
    order.clear();
    for (int r = 0; r < nb; ++r) {
        kept[r].score_lm = 0.0;
        if (a.ng) {
            CgHyp& h = hy[cur][r];
            if (h.carry.pw != 1) cg_push_word(&h, h.close_wid, h.close_add);
            h.slm += cg_word_add(*a.ng, h, a.ng->eos, a.lm_scale);
            kept[r].score_lm = h.slm;
        }
        if (a.bias) kept[r].score_lm = st[cur][r].banked;
        key[r] = cs_key(kept[r].score, kept[r].score_lm, a.lp, kept[r].len);
        order.push_back(r);
    }
    if (a.ng || a.bias) std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] > key[y]; });
    a.out.n_out[b] = nb;
    for (int r = 0; r < W; ++r)
        cs_write_row(a.out, (long long)b * W + r, hpar.data(), htok.data(), 0, W, steps, r < nb ? order[r] : -1, kept[r < nb ? order[r] : 0]);
}
