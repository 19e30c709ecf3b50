// AST beam search with word n-gram fusion: the step functions the kernels (ast_ngram.hip) and the serial host entry
// (cn_ast_ngram_adds_host; tools/ast_ngram_check.cpp builds it with a plain C++ compiler under sanitizers) are both made of.
// The contract is in include/cassnat_hip_ast_ngram.h.
//
// A hypothesis is a row of word-piece ids (no sos).  Ids equal to eos and ids outside [0, vocab) contribute no piece; the others are
// glued with the ranker's piece monoid (ngram_core.h), a piece that begins with a separator closing the word before it.  What the
// walk leaves behind is an AnState: the carry of the open word (pw == 1: none), the last NG_HIST closed word ids (<s> in front) and
// their count.  From it the two numbers a step needs derive with at most 15 + 15 independent table probes (ng_probe), summed in
// ng_word_score's order (ng_probe_score):
//   close32 = score(open word | history), end32 = score(</s> | history [+ open word])
//   a_word  = open ? close32 : 0,          a_eos = open ? fl32(close32 + end32) : end32
// and the term of a candidate token c is a_eos if c == eos, a_word if the piece c begins with a separator, else 0.
#pragma once
#include "../../include/cassnat_hip_ast_ngram.h"
#include "ngram_core.h"

constexpr int AN_CLOSE = 0, AN_END = NG_TASKS;  // first probe of the open word's score / of </s>'s in an NgProbe[2 * NG_TASKS]

struct AnState {
    NgPiece carry;              // the open word
    int32_t hist[NG_HIST + 2];  // the last NG_HIST closed word ids, oldest first (<s> in front), then room for the open word's id
    int32_t nwords;             // words closed so far
};

NG_HD bool an_real(const cn_ngram_desc& d, int32_t t, int32_t eos) { return t != eos && t >= 0 && t < d.vocab; }

NG_HD int an_context(const cn_ngram_desc& d, int nwords) { return nwords + 1 < d.order - 1 ? nwords + 1 : d.order - 1; }

NG_HD void an_init(const cn_ngram_desc& d, AnState* s) {
    s->carry = ng_piece(d, 0, false);
    for (int i = 0; i < NG_HIST + 2; ++i) s->hist[i] = d.bos;
    s->nwords = 0;
}

NG_HD void an_push_word(AnState* s, int32_t w) {
    for (int i = 0; i + 1 < NG_HIST; ++i) s->hist[i] = s->hist[i + 1];
    s->hist[NG_HIST - 1] = w;
    ++s->nwords;
}

// one more id of the row (the serial walk; the kernel reaches the same state with a segmented scan)
NG_HD void an_advance(const cn_ngram_desc& d, AnState* s, int32_t t, int32_t eos) {
    if (!an_real(d, t, eos)) return;
    const NgPiece pc = ng_piece(d, t, true);
    if (pc.starts && s->carry.pw != 1) an_push_word(s, ng_word_id(d, s->carry.h));
    s->carry = ng_combine(s->carry, pc);
}

// What probe `task` of 0 .. 2 * NG_TASKS - 1 looks up, given the walked state with hist[NG_HIST] = id of the open word (if any):
// tasks AN_CLOSE + t score the open word behind the history, tasks AN_END + t score </s> behind the history plus the open word.
NG_HD void an_probe(const cn_ngram_desc& d, const AnState& s, int task, NgProbe* out) {
    const bool open = s.carry.pw != 1;
    out->prob = 0.f, out->bo = 0.f, out->found = 0;
    if (task < AN_END) {
        if (open && task < NG_TASKS - 1) ng_probe(d, s.hist + NG_HIST, an_context(d, s.nwords), s.hist[NG_HIST], task, out);
    } else if (task - AN_END < NG_TASKS - 1) {
        const int shift = open ? 1 : 0;
        ng_probe(d, s.hist + NG_HIST + shift, an_context(d, s.nwords + shift), d.eos, task - AN_END, out);
    }
}

// adds = (a_word, a_eos) from the 2 * NG_TASKS probes
NG_HD void an_adds(const cn_ngram_desc& d, const AnState& s, const NgProbe* pr, float* adds) {
    const bool open = s.carry.pw != 1;
    const int shift = open ? 1 : 0;
    const float end32 = ng_probe_score(pr + AN_END, an_context(d, s.nwords + shift));
    if (open) {
        const float close32 = ng_probe_score(pr + AN_CLOSE, an_context(d, s.nwords));
        adds[0] = close32;
        adds[1] = close32 + end32;
    } else {
        adds[0] = 0.f;
        adds[1] = end32;
    }
}

NG_HD float an_term(const unsigned char* starts, const float* adds, int32_t eos, int32_t c, int32_t V) {
    if (c == eos) return adds[1];
    return (c >= 0 && c < V && starts[c]) ? adds[0] : 0.f;
}

// ---- host only -------------------------------------------------------------------------------------------------------------------
// adds of one row of n ids, every pointer a host pointer
inline void an_adds_row_host(const cn_ngram_desc& d, const int32_t* tok, int n, int32_t eos, float* adds) {
    AnState s;
    an_init(d, &s);
    for (int i = 0; i < n; ++i) an_advance(d, &s, tok[i], eos);
    if (s.carry.pw != 1) s.hist[NG_HIST] = ng_word_id(d, s.carry.h);
    NgProbe pr[2 * NG_TASKS];
    for (int t = 0; t < 2 * NG_TASKS; ++t) an_probe(d, s, t, &pr[t]);
    an_adds(d, s, pr, adds);
}
