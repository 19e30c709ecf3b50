// CTC prefix beam search that merges candidates by prefix: the step added to the shared search (ctc_search.h) between forming a
// frame's candidates and ranking them - duplicate labels, the identity of label sequences on the back-pointer chains, the fold.
// The contract is in include/cassnat_hip_ctc_merge.h.  The kernel (ctc_beam.hip, MERGE = true) and the serial host search
// (ctc_search_host.h with `merge` set; cn_ctc_merged_beam_host; tools/ctc_merge_check.cpp builds it with a plain C++ compiler under
// sanitizers) share the candidate, key, fold and state functions; they decide identity in two independent ways: the kernel by ids, a
// hash and a walk of the back-pointer chains, the host search by comparing the label vectors it keeps.
#pragma once
#include <cstdint>

#include "../../include/cassnat_hip_ctc_merge.h"
#include "ctc_bias_search.h"
#include "ctc_ngram_search.h"

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
