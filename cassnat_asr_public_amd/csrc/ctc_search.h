// CTC prefix beam search, the parts every variant shares, written once as __host__ __device__ code (a plain C++ compiler reads it
// too: tools/ctc_ngram_check.cpp).  Reference: ctc_beam_decode (src/utils/beam_decode.py:8-93).
//
// ctc_beam_decode is a per-frame loop over a Python list of hypotheses: every kept hypothesis yields one "stay" candidate (blank or a
// repetition of its last label) and one candidate per pruned label of the frame; the candidates are NOT merged by prefix; a stable
// descending sort by score_ctc + score_lm + ctc_lp * len(hyp) keeps `ctc_beam` of them.  Frames past src_size and frames whose blank
// probability exceeds 0.95 are skipped.  All scores are Python floats (float64) made of float32 log-posteriors.
//
// The variants differ in how score_lm is formed and in where they keep their state, and in nothing else:
//   ctc_beam.hip     no LM (score_lm = 0), the word n-gram model (ctc_ngram_search.h) and the phrase-biasing automaton
//                    (ctc_bias_search.h), each with or without merging by prefix (ctc_merge_search.h): one launch, the frame loop
//                    inside, state in LDS; what to run is one CtcSearchArgs, below
//   ctc_lm.hip       the TransformerLM in the loop: one launch per processed frame, state in global memory
//   ctc_search_host  every policy of ctc_beam.hip once more, serial, with std::stable_sort (ctc_search_host.h)
// Each forms score_lm itself and takes from here: the frame predicate, the CTC half of a candidate, the sort key, the stable top-W as
// a counting rank, and the unrolling of the (parent, label) back-pointers into the output rows.  Integer / ordering work: the
// hypotheses are those of the reference wherever two keys are not within an ulp of each other.
#pragma once
#include <cmath>

#include "../../include/cassnat_hip_ctc_bias.h"
#include "ngram_core.h"  // NG_HD, cn_ngram_desc

#define CS_LOGZERO (-1e10)
constexpr int CS_MAX_BEAM = 32, CS_MAX_PRUNE = 32;

struct CtcBeamOut {
    int* hyp = nullptr;          // [B][W][Lmax] labels (no sos), zeros behind
    int* hyp_len = nullptr;      // [B][W]
    double* score = nullptr;     // [B][W] score_ctc
    double* score_lm = nullptr;  // [B][W] (null: the search has none)
    double* p_blk = nullptr;     // [B][W]
    double* p_nblk = nullptr;
    int* n_out = nullptr;        // [B] hypotheses kept
    int Lmax = 0;
};
struct CtcBeamArgs {
    const float* logp = nullptr;        // [B][Tp][V] CTC log-posteriors of ALL frames
    const int* top_idx = nullptr;       // [B][Tp][P] pruned labels per frame, in list order (may be null when P = 0)
    const float* size_ratio = nullptr;  // [B]
    int B = 0, Tp = 0, V = 0, P = 0, W = 0, blank = 0;
    double lp = 0.0;                       // args.ctc_lp
    unsigned char* hist_parent = nullptr;  // [B][Tp][W] scratch
    int* hist_tok = nullptr;               // [B][Tp][W] scratch
    CtcBeamOut out;
};

inline CtcBeamArgs ctc_beam_args(const float* logp, const int* top_idx, const float* size_ratio, int B, int Tp, int V, int beam, int pruning,
                                 int blank, double lp, const CtcBeamOut& out) {
    CtcBeamArgs a;
    a.logp = logp, a.top_idx = top_idx, a.size_ratio = size_ratio;
    a.B = B, a.Tp = Tp, a.V = V, a.P = pruning, a.W = beam, a.blank = blank, a.lp = lp;
    a.out = out;
    return a;
}

// One search of ctc_beam.hip or of its serial twin: the shared arguments, how score_lm is formed (neither descriptor: it is 0) and
// whether candidates that spell the same labels are merged.  out.score_lm may be null only without fusion and without merging.
struct CtcSearchArgs : CtcBeamArgs {
    const cn_ngram_desc* ng = nullptr;  // at most one of ng / bias
    double lm_scale = 0.0;              // (n-gram) ctc_lm_weight * ln(10)
    const cn_bias_desc* bias = nullptr;
    bool merge = false;
};
inline CtcSearchArgs ctc_search_args(const CtcBeamArgs& search, const cn_ngram_desc* ng = nullptr, double lm_scale = 0.0,
                                     const cn_bias_desc* bias = nullptr, bool merge = false) {
    CtcSearchArgs a;
    static_cast<CtcBeamArgs&>(a) = search;
    a.ng = ng, a.lm_scale = lm_scale, a.bias = bias, a.merge = merge;
    return a;
}

inline CtcBeamOut ctc_beam_out(int* hyp, int hyp_cap, int* hyp_len, double* score, double* score_lm, double* p_blk, double* p_nblk, int* nbeam) {
    CtcBeamOut o;
    o.hyp = hyp, o.Lmax = hyp_cap, o.hyp_len = hyp_len, o.score = score, o.score_lm = score_lm, o.p_blk = p_blk, o.p_nblk = p_nblk, o.n_out = nbeam;
    return o;
}

// null when a search of these sizes can run, else what is wrong (Tp < 1: not known yet, hyp_cap is not looked at)
inline const char* cs_check_limits(int W, int P, int Tp, int hyp_cap) {
    if (W < 1 || W > CS_MAX_BEAM || P < 0 || P > CS_MAX_PRUNE) return "need 1 <= ctc_beam <= 32 and 0 <= ctc_pruning <= 32";
    if (Tp >= 1 && hyp_cap < Tp + 1) return "hyp_cap must be at least T' + 1";
    return nullptr;
}

// dynamic LDS of a frame step over W hypotheses and NC = W * (P + 1) candidates.  Doubles: 3 per hypothesis; key, p_blk, p_nblk,
// score_ctc (and score_lm) per candidate.  Ints: per hypothesis length and last label, per candidate parent, label, length and last
// label (ctc_lm_frame_kernel: 4 and 2).  The bias policy adds a double and an int per candidate: the state the candidate arrives at.
inline size_t cs_lds_bytes(int W, int P, bool with_lm, int ints_hyp = 2, int ints_cand = 4, int more_doubles_cand = 0) {
    const size_t NC = (size_t)W * (P + 1);
    return (3 * (size_t)W + ((with_lm ? 5 : 4) + more_doubles_cand) * NC) * 8 + (ints_hyp * (size_t)W + ints_cand * NC) * 4 + 64;
}

NG_HD double cs_logaddexp(double x, double y) {  // numpy's npy_logaddexp
    if (x == y) return x + 0.693147180559945309417232121458176568;
    const double tmp = x - y;
    if (tmp > 0) return x + log1p(exp(-tmp));
    if (tmp <= 0) return y + log1p(exp(tmp));
    return tmp;
}

// src_size = (ratio * T').long(): fp32 product, truncation (beam_decode.py:22); frames t <= src_size are looked at (the reference
// does process frame t == src_size), so everything from T' - 1 up means "all" and everything below 0 "none" (a ratio that is no
// number: none)
NG_HD int cs_src_size(float ratio, int Tp) {
    const float r = ratio * (float)Tp;
    return r >= (float)Tp ? Tp : (r > -1.f ? (int)r : -1);
}

// a frame is skipped when torch.exp of its float32 blank log-posterior exceeds the double 0.95
NG_HD bool cs_skip_frame(float pblank) { return (double)(float)exp((double)pblank) > 0.95; }

// The CTC half of a candidate of hypothesis k (p_b, p_nb, last label or -1, length): `stay` is blank or a repetition of the last
// label, else label c is appended (blank or an id outside [0, V): no candidate, par = -1).  row: the frame's V log-posteriors.
struct CsCand {
    double pb, pnb, tot;      // p_blk, p_nblk, score_ctc
    int par, tok, len, last;  // par -1: not a candidate; tok -1: stay
};
NG_HD CsCand cs_candidate(const float* row, int V, int blank, int k, bool stay, int c, double p_b, double p_nb, int last, int len) {
    CsCand r;
    r.par = -1, r.tok = -1, r.len = 0, r.last = -1;
    r.pb = r.pnb = r.tot = CS_LOGZERO;
    if (stay) {
        r.pnb = len > 0 ? p_nb + (double)row[last] : CS_LOGZERO;
        const double pt = (double)row[blank];
        r.pb = cs_logaddexp(p_b + pt, p_nb + pt);
        r.tot = cs_logaddexp(r.pb, r.pnb);
        r.par = k, r.len = len, r.last = last;
    } else if (c >= 0 && c != blank && c < V) {
        const double pt = (double)row[c];
        r.pnb = (c != last) ? cs_logaddexp(p_b + pt, p_nb + pt) : p_b + pt;
        r.tot = cs_logaddexp(CS_LOGZERO, r.pnb);
        r.par = k, r.tok = c, r.len = len + 1, r.last = c;
    }
    return r;
}

// x['score_ctc'] + x['score_lm'] + length_penalty * len(x['hyp']) as Python forms it: the product rounded on its own.  The empty asm
// makes it opaque, so no compiler contracts it into the sum (hipcc does so even across __dmul_rn, a plain operator in HIP).
NG_HD double cs_key(double tot, double slm, double lp, int len) {
    double p = lp * (double)len;
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__ volatile("" : "+v"(p));
#else
    __asm__ volatile("" : "+m"(p));
#endif
    return (tot + slm) + p;
}

// The stable descending order as a count: how many of the ncand candidates sort before candidate i - a larger key, or the same key
// at an earlier position; entries with par < 0 are no candidates.  The W best are the ones with rank < W, rank their new slot.
NG_HD int cs_rank(const double* key, const int* par, int ncand, int i) {
    const double ki = key[i];
    int rank = 0;
#pragma unroll 4
    for (int j = 0; j < ncand; ++j) {  // (no branch inside: the loads of several j are in flight together)
        const double kj = key[j];
        rank += (par[j] >= 0) & ((kj > ki) | ((kj == ki) & (j < i)));
    }
    return rank;
}

NG_HD int cs_count_valid(const int* par, int ncand, int W) {  // hypotheses the frame keeps
    int valid = 0;
    for (int j = 0; j < ncand; ++j) valid += par[j] >= 0 ? 1 : 0;
    return valid < W ? valid : W;
}

// What a kept hypothesis hands to its output row
struct CsKept {
    double score, score_lm, p_blk, p_nblk;
    int len;
};

// Row o (= utterance * W + destination slot) of the outputs.  src >= 0: the hypothesis in slot src after `steps` processed frames,
// its labels unrolled from the back-pointers hist_parent / hist_tok (entry (step, slot) of the utterance at step * W + slot behind
// `hist_base` entries), zeros behind them.  src < 0: the row of an unused slot.
NG_HD void cs_write_row(const CtcBeamOut& out, long long o, const unsigned char* hist_parent, const int* hist_tok, long long hist_base, int W,
                        int steps, int src, const CsKept& kept) {
    int* h = out.hyp + o * out.Lmax;
    if (src < 0) {
        for (int i = 0; i < out.Lmax; ++i) h[i] = 0;
        out.hyp_len[o] = 0;
        out.score[o] = out.p_blk[o] = out.p_nblk[o] = CS_LOGZERO;
        if (out.score_lm) out.score_lm[o] = 0.0;
        return;
    }
    int pos = kept.len - 1, at = src;
    for (int st = steps - 1; st >= 0; --st) {
        const long long e = hist_base + (long long)st * W + at;
        const int tok = hist_tok[e];
        if (tok >= 0) {
            if (pos >= 0 && pos < out.Lmax) h[pos] = tok;
            --pos;
        }
        at = hist_parent[e];
    }
    for (int i = kept.len < 0 ? 0 : kept.len; i < out.Lmax; ++i) h[i] = 0;
    out.hyp_len[o] = kept.len;
    out.score[o] = kept.score;
    if (out.score_lm) out.score_lm[o] = kept.score_lm;
    out.p_blk[o] = kept.p_blk;
    out.p_nblk[o] = kept.p_nblk;
}
