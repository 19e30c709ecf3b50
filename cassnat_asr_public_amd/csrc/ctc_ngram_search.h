// CTC prefix beam search with word n-gram fusion: score_lm of the shared search (ctc_search.h) formed from an ARPA model - the n-gram
// state of a hypothesis and its update.  The kernel (ctc_beam.hip) and the serial host search (ctc_search_host.h; cn_ctc_ngram_beam_host;
// tools/ctc_ngram_check.cpp builds it with a plain C++ compiler under sanitizers) are made of the same functions.
//
// The contract is in include/cassnat_hip_ctc_ngram.h.  A hypothesis carries the piece-monoid carry of its open
// word, its last NG_HIST word ids (<s> in front), its word count, and - looked up once, when the open word changes - the id of the
// open word and what closing it adds: double(ng_word_score(history, word)) * lm_scale.  A candidate that appends a real piece which
// begins with a separator to a hypothesis with a non-empty open word closes that word and adds the parent's cached value; every
// other candidate adds nothing.  Labels equal to CG_DROP are left out of the gluing, as the ranker does with drop_id = 2.
#pragma once
#include "../../include/cassnat_hip_ctc_ngram.h"
#include "ctc_search.h"

constexpr int CG_DROP = 2;

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
// double(score of word w behind h's history) * lm_scale, from the probes
inline double cg_word_add(const cn_ngram_desc& d, const CgHyp& h, int32_t w, double lm_scale) {
    NgProbe pr[NG_TASKS];
    const int c = cg_context(d, h);
    for (int t = 0; t < NG_TASKS - 1; ++t) ng_probe(d, h.hist + NG_HIST, c, w, t, &pr[t]);
    return (double)ng_probe_score(pr, c) * lm_scale;
}
