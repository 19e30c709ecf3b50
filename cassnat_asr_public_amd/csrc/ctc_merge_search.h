// CTC prefix beam search that merges candidates by prefix: the step added to the shared search (ctc_search.h) between forming a
// frame's candidates and ranking them - duplicate labels, the identity of label sequences on the back-pointer chains, the fold - and
// the serial host search (cn_ctc_merged_beam_host; tools/ctc_merge_check.cpp builds it with a plain C++ compiler under sanitizers).
// The contract is in include/cassnat_hip_ctc_merge.h.  The kernel (ctc_beam.hip, MERGE = true) and the host search share the
// candidate, key, fold and state functions; they decide identity in two independent ways: the kernel by ids, a hash and a walk of the
// back-pointer chains, the host search by comparing the label vectors it keeps.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cassnat_hip_ctc_merge.h"
#include "ctc_bias_search.h"
#include "ctc_ngram_search.h"

struct CtcMergeArgs : CtcBeamArgs {  // (out.score_lm is written)
    const cn_ngram_desc* ng = nullptr;  // at most one of ng / bias
    double lm_scale = 0.0;
    const cn_bias_desc* bias = nullptr;
};
inline CtcMergeArgs ctc_merge_args(const cn_ngram_desc* ng, double lm_scale, const cn_bias_desc* bias, const CtcBeamArgs& search) {
    CtcMergeArgs a;
    static_cast<CtcBeamArgs&>(a) = search;
    a.ng = ng, a.lm_scale = lm_scale, a.bias = bias;
    return a;
}
#ifdef __HIPCC__
int launch_ctc_merged_beam(const CtcMergeArgs& a, hipStream_t s);
#endif

// label j - 1 of the frame's pruned list `top` (j >= 1; c is top[j - 1]), or -1 where the list has it at an earlier position
NG_HD int cm_dedup(const int* top, int j, int c) {
    bool dup = false;
    for (int q = 0; q + 1 < j; ++q) dup |= top[q] == c;
    return dup ? -1 : c;
}

// the hash of a label sequence with label c appended (the empty sequence: 0); a pre-filter, it never decides
NG_HD uint32_t cm_hash(uint32_t h, int c) {
    h = (h ^ (uint32_t)c) * 0x9E3779B1u + 0x7F4A7C15u;
    return h ^ (h >> 15);
}

// The next label on the chain of the hypothesis in slot *slot after step *st, walking towards the start; -1: the chain has ended.
// Moves (*st, *slot) to the hypothesis the label was appended to.  At most *st + 1 entries are read.
NG_HD int cm_chain_next(const unsigned char* hist_parent, const int* hist_tok, int W, int* st, int* slot) {
    while (*st >= 0) {
        const long long e = (long long)*st * W + *slot;
        const int tok = hist_tok[e];
        *slot = hist_parent[e];
        --*st;
        if (tok >= 0) return tok;
    }
    return -1;
}

// seq(kp) == seq(k) + c for the hypotheses in slots kp and k after `steps` processed frames, from the back-pointers alone (entry
// (step, slot) at step * W + slot).  Both chains are read label by label from their ends; it stops at the first label that
// differs, when both have ended, or when both have arrived at the same entry (the same hypothesis: the same labels before).
NG_HD bool cm_same_sequence(const unsigned char* hist_parent, const int* hist_tok, int W, int steps, int kp, int k, int c) {
    int sa = steps - 1, a = kp, sb = steps - 1, b = k;
    int tb = c;                          // the extension's own label comes first
    for (int n = 0; n <= steps; ++n) {   // (a chain has at most `steps` labels)
        const int ta = cm_chain_next(hist_parent, hist_tok, W, &sa, &a);
        if (ta != tb) return false;
        if (ta < 0 || (sa == sb && a == b)) return true;
        tb = cm_chain_next(hist_parent, hist_tok, W, &sb, &b);
    }
    return false;
}

// the stay candidate with the extension's p_nblk folded in
NG_HD void cm_fold(double pb_stay, double* pnb_stay, double* tot_stay, double pnb_ext) {
    *pnb_stay = cs_logaddexp(*pnb_stay, pnb_ext);
    *tot_stay = cs_logaddexp(pb_stay, *pnb_stay);
}

// ---- host only -------------------------------------------------------------------------------------------------------------------
inline cn_bias_desc cm_no_bias() {  // the root alone: a valid descriptor whose tables are not read
    cn_bias_desc d = {};
    d.slots = 1, d.nodes = 0, d.hash_bits = 32;
    return d;
}

// "" when the arguments can be searched, else what is wrong: cg_check's / cb_check's refusals
inline std::string cm_check(const CtcMergeArgs& a, bool need_scratch) {
    if (a.ng && a.bias) return "at most one of the n-gram and the bias descriptor may be set";
    if (a.ng) return cg_check(ctc_ngram_args(*a.ng, a.lm_scale, a), need_scratch);
    return cb_check(ctc_bias_args(a.bias ? *a.bias : cm_no_bias(), a), need_scratch);
}

// utterance b of `a`, every pointer a host pointer; the back-pointers are kept here, a.hist_parent / a.hist_tok are not used.  The
// order comes from std::stable_sort and identity from the label vectors: the independent check of cs_rank and of the kernel's
// identity test.
inline void cm_search_host(const CtcMergeArgs& a, int b) {
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
        for (int j = 1; j <= P; ++j) lab[j - 1] = cm_dedup(top + (long long)t * P, j, top[(long long)t * P + (j - 1)]);
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
            if (x.c.tok < 0) continue;
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
    // the steps after the last frame are the unmerged searches'; one more stable sort by the same key
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
