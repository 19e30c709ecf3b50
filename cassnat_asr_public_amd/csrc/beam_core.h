// What the two token-level beam searches on the device share (ast.hip: Transformer.beam_decode; natlm.hip: the CASS-NAT finish
// loop with a fused LM): the tables of a slot (kernels.h: BeamTables), the ranking key, the stable rank over the keys and the
// copy that makes a new slot's row from its parent's.  Device functions only - how a step's candidates come about differs
// (finished hypotheses, per-beam top-bw of K and unused slots there; a fixed bw * bw list and ended utterances here), so each
// search keeps its own update kernel around them.
#pragma once
#include "kernels.h"

// slot s of buffer p at the start of a search: [sos], every position computed in the slot itself
__device__ __forceinline__ void beam_init_row(const BeamTables& st, int p, int s, int L, int sos, int pad) {
    for (int t = 0; t < L; ++t) {
        st.tok[p][(long long)s * L + t] = t == 0 ? sos : pad;
        st.anc[p][(long long)s * L + t] = s;
        st.keyok[p][(long long)s * L + t] = (t == 0 && sos != pad) ? 1 : 0;
    }
    st.score[p][s] = 0.0;
}

// score + (len(hyp) - 1) * length_penalty as Python computes it (double, the product rounded before the sum), or the score alone
__device__ __forceinline__ double beam_key(double score, int len_minus_1, double lp, int use_lp) {
    return use_lp ? score + cn_mul_rn((double)len_minus_1, lp) : score;
}

// rank of candidate e among keys[0 .. n): descending, ties in list order (Python's stable sort).  A NaN key ranks first against
// everything and nothing ranks before it: what each kernel's newslot initialiser is there for.
__device__ __forceinline__ int beam_rank(const double* keys, int n, int e) {
    const double k = keys[e];
    int r = 0;
    for (int e2 = 0; e2 < n; ++e2) r += (keys[e2] > k) || (keys[e2] == k && e2 < e);
    return r;
}

// Row of the new slot sn in buffer cur ^ 1 from its parent so in buffer cur, by the whole workgroup (nthreads threads, this one
// tid).  grown: the hypothesis gained `token` at position wpos this step (`step` = the position whose K | V the step computed in
// the parent's slot), so the ancestor of position step is so and position step + 1 will be computed in sn.  A live hypothesis at
// step `step` holds step + 1 tokens, so wpos == step + 1 in both loops; the searches still pass their own expression of it (the
// parent's length / step + 1), since the kernel-test entries take a length and a step that need not agree.
__device__ __forceinline__ void beam_write_row(const BeamTables& st, int cur, int L, int so, int sn, bool grown, int wpos, int step,
                                               int token, int pad, int tid, int nthreads) {
    const int nxt = cur ^ 1;
    for (int t = tid; t < L; t += nthreads) {
        int tk = st.tok[cur][(long long)so * L + t], an = st.anc[cur][(long long)so * L + t];
        unsigned char ko = st.keyok[cur][(long long)so * L + t];
        if (grown) {
            if (t == wpos) {
                tk = token;
                ko = token != pad;  // tgt_mask = (ys != padding_idx): a blank inside the prefix is masked for later positions
            }
            if (t == step) an = so;      // position `step` was computed in the parent's slot this step
            if (t == step + 1) an = sn;  // the next position will be computed in this slot
        }
        st.tok[nxt][(long long)sn * L + t] = tk;
        st.anc[nxt][(long long)sn * L + t] = an;
        st.keyok[nxt][(long long)sn * L + t] = ko;
    }
}
