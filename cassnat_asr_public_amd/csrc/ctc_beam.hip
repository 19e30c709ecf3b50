// CTC prefix beam search - without a language model, and with a word n-gram model fused - and CTC forced (Viterbi) alignment for
// gfx950: the device half of `decode_type: ctc_only / ctc_att`.
//
// The search is ctc_search.h's (ctc_beam_decode, src/utils/beam_decode.py:8-93, called from src/tasks/cassnat_task.py:335-341): one
// workgroup of 256 per utterance, the frame loop inside the kernel, one candidate per thread (in rounds when there are more than
// 256), the stable top-W by counting rank, (parent, label) back-pointers per processed frame, unrolled at the end.  What to run is
// one CtcSearchArgs (ctc_search.h) behind one check (ctc_search_host.h) and one launcher, launch_ctc_beam; the serial twin of every
// search is ctc_search_host (cn_ctc_{ngram,bias,merged}_beam_host).  One kernel body, one instantiation per fusion policy:
//   ctc_beam_kernel<CS_FUSE_NONE>   score_lm = 0: `ctc_lm_weight: 0`.
//   ctc_beam_kernel<CS_FUSE_NGRAM>  score_lm = lm_scale * (the word scores of the words a hypothesis has closed): `rank_model: n-gram` with an
//                           ARPA model and ctc_lm_weight > 0 (ctc_ngram_search.h; the reference has no such search).  On top of the
//                           body above:
//     * the n-gram state of the kept hypotheses (CgHyp: carry, history, word count, score_lm and the cached value of closing the open
//       word) lives in LDS in two buffers: a winner writes slot `rank` of the other buffer from its parent's slot of this one;
//     * what closing a word adds depends on the parent alone, so table look-ups are per kept hypothesis whose open word changed (at
//       most W a frame), not per candidate: the winner's thread finds the word's id, then the up to 2 * order - 1 probes of the word's
//       score are spread over (hypothesis, task) threads and one thread per hypothesis adds them up in ng_word_score's float32 order;
//     * after the last frame every kept hypothesis adds its open word and </s>, and the beam is sorted once more by the same key.
//   ctc_beam_kernel<CS_FUSE_BIAS>   score_lm = the banked bonus of the listed phrases a hypothesis has completed plus the value of its open
//                           match (ctc_bias_search.h, include/cassnat_hip_ctc_bias.h; `--hip_bias`).  On top of the body above:
//     * (node, banked) of the kept hypotheses in static LDS, double buffered (2 * 32 * 16 bytes);
//     * what a label adds depends on the parent's node and on the label, so every candidate thread walks the hashed edges from its
//       parent's node (tables in global memory, ordinary loads) and leaves the state it arrives at in two more candidate arrays
//       (node, banked) of dynamic LDS: the winner copies them to slot `rank` of the other buffer and does not walk again;
//     * after the last frame every kept hypothesis gives up its open match and the beam is sorted once more by the same key.
//   Every probe loop is bounded by its table's slot count.
//   ctc_beam_kernel<FUSE, true>  any of the three policies, merging candidates that spell the same label sequence
//                           (ctc_merge_search.h, include/cassnat_hip_ctc_merge.h; `--hip_ctc_merge 1`; the reference does not merge).
//                           One more phase between the candidate phase and the rank phase, behind a barrier: every extension's thread
//                           looks for a kept hypothesis with its labels - (length, last label) and a 32-bit hash filter, an id link
//                           proves identity where there is one, else both back-pointer chains are walked - and folds its p_nblk into
//                           that hypothesis' stay candidate.  (id, prefix id, hash) per kept hypothesis in static LDS, double
//                           buffered; no scratch beyond the back-pointers.  The <FUSE, false> instantiations are the kernels above.
//
// viterbi_align (CassNAT.beam_path_align, src/models/cassnat.py:391-414, 272-353) is the max-product CTC forward pass over the
// blank-augmented label sequence in float32 followed by a sequential back-trace; here one workgroup per utterance with the two live
// alpha rows in LDS and the back-pointers in global memory; same float32 operation order, first-maximum-wins among the three
// predecessors (torch.max).
#include <type_traits>

#include "ctc_search_host.h"
#include "kernels.h"

enum { CS_FUSE_NONE = 0, CS_FUSE_NGRAM = 1, CS_FUSE_BIAS = 2 };  // how score_lm is formed

// what an instantiation keeps in static LDS (without fusion: nothing)
template <int FUSE>
struct CgLds {};
template <>
struct CgLds<CS_FUSE_BIAS> {
    CbState st[2][CS_MAX_BEAM];  // (node, banked), double buffered
};
template <>
struct CgLds<CS_FUSE_NGRAM> {
    CgHyp hyps[2][CS_MAX_BEAM];  // n-gram state, double buffered
    NgProbe probes[CS_MAX_BEAM * NG_TASKS];
    int wflag[CS_MAX_BEAM], wid[CS_MAX_BEAM];
};

// the word scores of hypotheses r < n with flag[r] set, word wid[r] behind hy[r]'s history: probes by (hypothesis, task) threads, then
// thread r returns double(score) * lm_scale (0 for the others).  All 256 threads call it; the caller puts a barrier behind its use.
__device__ __forceinline__ double cg_score_words(const cn_ngram_desc& d, const CgHyp* hy, const int* flag, const int* wid, int n,
                                                 NgProbe* probes, double lm_scale) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n * NG_TASKS; i += 256) {
        const int r = i / NG_TASKS, t = i - r * NG_TASKS;
        if (t < NG_TASKS - 1 && flag[r]) ng_probe(d, hy[r].hist + NG_HIST, cg_context(d, hy[r]), wid[r], t, &probes[i]);
    }
    __syncthreads();
    if (tid < n && flag[tid]) return (double)ng_probe_score(probes + tid * NG_TASKS, cg_context(d, hy[tid])) * lm_scale;
    return 0.0;
}

// what the merging instantiations keep per kept hypothesis in static LDS, double buffered: the id given when an extension was kept
// (stays inherit it), the id of the hypothesis it extended, the hash of its labels (include/cassnat_hip_ctc_merge.h)
template <bool MERGE>
struct CmLds {};
template <>
struct CmLds<true> {
    int id[2][CS_MAX_BEAM], pfx[2][CS_MAX_BEAM];
    uint32_t hash[2][CS_MAX_BEAM];
};

// what an instantiation takes by value: without fusion the shared arguments alone, else its descriptor behind them (out.score_lm is
// written)
struct CsNgramArgs : CtcBeamArgs {
    cn_ngram_desc d;
    double lm_scale = 0.0;  // ctc_lm_weight * ln(10)
};
struct CsBiasArgs : CtcBeamArgs {
    cn_bias_desc d;
};
template <int FUSE>
struct CsFuseArgs {
    using type = CtcBeamArgs;
};
template <>
struct CsFuseArgs<CS_FUSE_NGRAM> {
    using type = CsNgramArgs;
};
template <>
struct CsFuseArgs<CS_FUSE_BIAS> {
    using type = CsBiasArgs;
};

template <int FUSE, bool MERGE>
__global__ __launch_bounds__(256) void ctc_beam_kernel(typename CsFuseArgs<FUSE>::type a) {
    constexpr bool NGRAM = FUSE == CS_FUSE_NGRAM, BIAS = FUSE == CS_FUSE_BIAS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W = a.W, P = a.P, NC = W * (P + 1);
    // beam state
    double* pb = reinterpret_cast<double*>(smem);  // [W]
    double* pnb = pb + W;                          // [W]
    double* ckey = pnb + W;                        // [NC] candidates
    double* cpb = ckey + NC;
    double* cpnb = cpb + NC;
    double* ctot = cpnb + NC;
    double* cslm = ctot + NC;                      // (n-gram and bias only)
    double* cbank = cslm + (NGRAM || BIAS ? NC : 0);  // (bias only) the candidate's banked bonus
    double* ptot = cbank + (BIAS ? NC : 0);        // [W] score_ctc of the kept hypotheses
    int* blen = reinterpret_cast<int*>(ptot + W);  // [W]
    int* blast = blen + W;                         // [W] last label (-1: empty hypothesis)
    int* cpar = blast + W;                         // [NC] parent slot (-1: not a candidate)
    int* ctok = cpar + NC;                         // [NC] appended label (-1: stay)
    int* clen = ctok + NC;
    int* clast = clen + NC;
    int* cnode = clast + NC;  // (bias only) the candidate's automaton node
    __shared__ CgLds<FUSE> ng;
    __shared__ CmLds<MERGE> mg;
    __shared__ int s_nb, s_steps;

    const float* logp = a.logp + (long long)b * a.Tp * a.V;
    const int* top = a.top_idx + (long long)b * a.Tp * P;
    const long long hist = (long long)b * a.Tp * W;
    unsigned char* hpar = a.hist_parent + hist;
    int* htok = a.hist_tok + hist;
    const int ssz = cs_src_size(a.size_ratio[b], a.Tp);
    if (tid == 0) {
        pb[0] = 0.0;  // logone
        pnb[0] = CS_LOGZERO;
        ptot[0] = 0.0;
        blen[0] = 0;
        blast[0] = -1;
        if constexpr (NGRAM) cg_init(a.d, &ng.hyps[0][0]);
        if constexpr (BIAS) ng.st[0][0] = cb_init();
        if constexpr (MERGE) mg.id[0][0] = 0, mg.pfx[0][0] = -1, mg.hash[0][0] = 0u;
        s_nb = 1;
        s_steps = 0;
    }
    int cur = 0;
    [[maybe_unused]] int mcur = 0;  // (merging) the buffer of mg that holds the kept hypotheses
    __syncthreads();
    for (int t = 0; t < a.Tp; ++t) {
        if (t > ssz) continue;
        const float* row = logp + (long long)t * a.V;
        if (cs_skip_frame(row[a.blank])) continue;
        const int nb = s_nb, step = s_steps;
        const int ncand = nb * (P + 1);
        for (int i = tid; i < ncand; i += 256) {
            const int k = i / (P + 1), j = i - k * (P + 1);
            int c = j == 0 ? -1 : top[(long long)t * P + (j - 1)];
            if constexpr (MERGE) c = cm_dedup(top + (long long)t * P, j, c);
            const CsCand r = cs_candidate(row, a.V, a.blank, k, j == 0, c, pb[k], pnb[k], blast[k], blen[k]);
            double slm = 0.0;
            if constexpr (NGRAM) {
                if (r.par >= 0) slm = cg_candidate_slm(a.d, ng.hyps[cur][k], r.tok);
                cslm[i] = slm;
            }
            if constexpr (BIAS) {
                CbState st = cb_init();
                if (r.par >= 0) {
                    st = cb_step(a.d, ng.st[cur][k], r.tok);
                    slm = cb_slm(a.d, st);
                }
                cslm[i] = slm;
                cnode[i] = st.node;
                cbank[i] = st.banked;
            }
            cpar[i] = r.par;
            ctok[i] = r.tok;
            clen[i] = r.len;
            clast[i] = r.last;
            cpb[i] = r.pb;
            cpnb[i] = r.pnb;
            ctot[i] = r.tot;
            ckey[i] = cs_key(r.tot, slm, a.lp, r.len);
        }
        if constexpr (NGRAM) {
            if (tid < W) ng.wflag[tid] = 0;
        }
        __syncthreads();
        if constexpr (MERGE) {
            // the fold: an extension (k, c) that spells the labels of a kept hypothesis kp goes into kp's stay candidate.  At most one
            // extension folds into a given stay (the kept sequences differ pairwise, the list has no label twice): no two threads
            // write the same stay, and nobody reads a stay's p_nblk / score / key in this phase but the thread that folds into it.
            for (int i = tid; i < ncand; i += 256) {
                if (cpar[i] < 0 || ctok[i] < 0) continue;
                const int k = cpar[i], c = ctok[i], len1 = clen[i], idk = mg.id[mcur][k];
                const uint32_t h = cm_hash(mg.hash[mcur][k], c);
                int hit = -1;
                for (int kp = 0; kp < nb; ++kp) {
                    if (blen[kp] != len1 || blast[kp] != c) continue;
                    // kp was made by appending c to what k has been since: the same labels.  Else (a prefix dropped and made again
                    // has a new id) the chains decide, wherever the hash does not rule it out.
                    if (mg.pfx[mcur][kp] == idk || (mg.hash[mcur][kp] == h && cm_same_sequence(hpar, htok, W, step, kp, k, c))) {
                        hit = kp;
                        break;
                    }
                }
                if (hit >= 0) {
                    const int sty = hit * (P + 1);
                    cm_fold(cpb[sty], &cpnb[sty], &ctot[sty], cpnb[i]);
                    double slm = 0.0;
                    if constexpr (NGRAM || BIAS) slm = cslm[sty];
                    ckey[sty] = cs_key(ctot[sty], slm, a.lp, clen[sty]);
                    cpar[i] = -1;
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < ncand; i += 256) {
            if (cpar[i] < 0) continue;
            const int rank = cs_rank(ckey, cpar, ncand, i);
            if (rank < W) {
                pb[rank] = cpb[i];
                pnb[rank] = cpnb[i];
                ptot[rank] = ctot[i];
                blen[rank] = clen[i];
                blast[rank] = clast[i];
                hpar[(long long)step * W + rank] = (unsigned char)cpar[i];
                htok[(long long)step * W + rank] = ctok[i];
                if constexpr (NGRAM) {
                    CgHyp* h = &ng.hyps[cur ^ 1][rank];
                    if (cg_advance(a.d, ng.hyps[cur][cpar[i]], ctok[i], h) && h->carry.pw != 1) {
                        ng.wid[rank] = h->close_wid = ng_word_id(a.d, h->carry.h);
                        ng.wflag[rank] = 1;
                    }
                }
                if constexpr (BIAS) {
                    CbState st;
                    st.node = cnode[i], st.pad = 0, st.banked = cbank[i];
                    ng.st[cur ^ 1][rank] = st;
                }
                if constexpr (MERGE) {
                    const int k = cpar[i], c = ctok[i];
                    mg.id[mcur ^ 1][rank] = c < 0 ? mg.id[mcur][k] : step * W + rank + 1;
                    mg.pfx[mcur ^ 1][rank] = c < 0 ? mg.pfx[mcur][k] : mg.id[mcur][k];
                    mg.hash[mcur ^ 1][rank] = c < 0 ? mg.hash[mcur][k] : cm_hash(mg.hash[mcur][k], c);
                }
            }
        }
        // (pb / pnb / blen / blast were only read in the candidate phase above, behind the barrier: safe to overwrite)
        if (tid == 0) {
            s_nb = cs_count_valid(cpar, ncand, W);
            s_steps = step + 1;
        }
        __syncthreads();
        if constexpr (NGRAM) {
            cur ^= 1;
            const int kept = s_nb;
            const double add = cg_score_words(a.d, ng.hyps[cur], ng.wflag, ng.wid, kept, ng.probes, a.lm_scale);
            if (tid < kept && ng.wflag[tid]) ng.hyps[cur][tid].close_add = add;
            __syncthreads();
        }
        if constexpr (BIAS) cur ^= 1;
        if constexpr (MERGE) mcur ^= 1;
    }
    const int nb = s_nb, steps = s_steps;
    int out = tid;  // the slot a kept hypothesis is written at
    if constexpr (NGRAM) {
        // the open word, then </s>, and one more stable sort by the same key
        if (tid < nb) {
            CgHyp* h = &ng.hyps[cur][tid];
            if (h->carry.pw != 1) cg_push_word(h, h->close_wid, h->close_add);
            ng.wflag[tid] = 1;
            ng.wid[tid] = a.d.eos;
        }
        __syncthreads();
        const double add = cg_score_words(a.d, ng.hyps[cur], ng.wflag, ng.wid, nb, ng.probes, a.lm_scale);
        if (tid < nb) {
            ng.hyps[cur][tid].slm += add;
            ckey[tid] = cs_key(ptot[tid], ng.hyps[cur][tid].slm, a.lp, blen[tid]);
            cpar[tid] = tid;
        }
        __syncthreads();
        if (tid < nb) out = cs_rank(ckey, cpar, nb, tid);
    }
    if constexpr (BIAS) {
        // the open match is given up, and one more stable sort by the same key
        if (tid < nb) {
            ckey[tid] = cs_key(ptot[tid], ng.st[cur][tid].banked, a.lp, blen[tid]);
            cpar[tid] = tid;
        }
        __syncthreads();
        if (tid < nb) out = cs_rank(ckey, cpar, nb, tid);
    }
    // one thread per slot: a kept hypothesis unrolls its back-pointers
    if (tid == 0) a.out.n_out[b] = nb;
    if (tid < W) {
        CsKept kept = {};
        if (tid < nb) {
            kept.score = ptot[tid], kept.p_blk = pb[tid], kept.p_nblk = pnb[tid], kept.len = blen[tid];
            if constexpr (NGRAM) kept.score_lm = ng.hyps[cur][tid].slm;
            if constexpr (BIAS) kept.score_lm = ng.st[cur][tid].banked;
        }
        cs_write_row(a.out, (long long)b * W + out, a.hist_parent, a.hist_tok, hist, W, steps, tid < nb ? tid : -1, kept);
    }
}

template <int FUSE, bool MERGE, class Args>
static int launch_beam(const Args& a, hipStream_t s) {
    constexpr bool BIAS = FUSE == CS_FUSE_BIAS;
    static CnAttrOnce attr_once;  // (one per instantiation)
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        CN_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_beam_kernel<FUSE, MERGE>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_once.mark(attr_dev);
    }
    const size_t lds = cs_lds_bytes(a.W, a.P, FUSE != CS_FUSE_NONE, 2, BIAS ? 5 : 4, BIAS ? 1 : 0);
    hipLaunchKernelGGL((ctc_beam_kernel<FUSE, MERGE>), dim3(a.B), dim3(256), lds, s, a);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// every search of this file: the one check, then the instantiation of the descriptor's policy, merging or not
int launch_ctc_beam(const CtcSearchArgs& a, hipStream_t s) {
    if (!a.ng && !a.bias && !a.merge && a.B <= 0) return 0;
    const std::string bad = ctc_search_check(a, true);
    if (!bad.empty()) {
        cn_set_error("ctc_beam: " + bad);
        return -1;
    }
    if (a.ng) {
        CsNgramArgs k;
        static_cast<CtcBeamArgs&>(k) = a;
        k.d = *a.ng, k.lm_scale = a.lm_scale;
        return a.merge ? launch_beam<CS_FUSE_NGRAM, true>(k, s) : launch_beam<CS_FUSE_NGRAM, false>(k, s);
    }
    if (a.bias) {
        CsBiasArgs k;
        static_cast<CtcBeamArgs&>(k) = a;
        k.d = *a.bias;
        return a.merge ? launch_beam<CS_FUSE_BIAS, true>(k, s) : launch_beam<CS_FUSE_BIAS, false>(k, s);
    }
    const CtcBeamArgs& k = a;
    return a.merge ? launch_beam<CS_FUSE_NONE, true>(k, s) : launch_beam<CS_FUSE_NONE, false>(k, s);
}

// The serial search on the host (ctc_search_host.h): every pointer a host pointer, no GPU call.  `who` refuses with "null argument"
// where its own descriptor is mandatory and missing.
static int ctc_beam_host(const char* who, bool desc_missing, const CtcSearchArgs& a) {
    const std::string bad = desc_missing ? "null argument" : ctc_search_check(a, false);
    if (!bad.empty()) {
        cn_set_error(std::string(who) + ": " + bad);
        return -1;
    }
    for (int b = 0; b < a.B; ++b) ctc_search_host(a, b);
    return 0;
}

extern "C" int cn_ctc_ngram_beam_host(const cn_ngram_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                                      int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, double lm_scale,
                                      int32_t blank, int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm,
                                      double* p_blk, double* p_nblk, int32_t* nbeam) {
    return ctc_beam_host("cn_ctc_ngram_beam_host", !desc,
                         ctc_search_args(ctc_beam_args(logp, top_idx, size_ratio, B, Tp, V, beam, pruning, blank, length_penalty,
                                                       ctc_beam_out(hyp, hyp_cap, hyp_len, score, score_lm, p_blk, p_nblk, nbeam)),
                                         desc, lm_scale));
}

extern "C" int cn_ctc_bias_beam_host(const cn_bias_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                                     int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, int32_t blank,
                                     int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm, double* p_blk,
                                     double* p_nblk, int32_t* nbeam) {
    return ctc_beam_host("cn_ctc_bias_beam_host", !desc,
                         ctc_search_args(ctc_beam_args(logp, top_idx, size_ratio, B, Tp, V, beam, pruning, blank, length_penalty,
                                                       ctc_beam_out(hyp, hyp_cap, hyp_len, score, score_lm, p_blk, p_nblk, nbeam)),
                                         nullptr, 0.0, desc));
}

// (merging by prefix, include/cassnat_hip_ctc_merge.h: both descriptors may be null)
extern "C" int cn_ctc_merged_beam_host(const cn_ngram_desc* ngram_desc, double lm_scale, const cn_bias_desc* bias_desc, const float* logp,
                                       const int32_t* top_idx, const float* size_ratio, int32_t B, int32_t Tp, int32_t V, int32_t beam,
                                       int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp, int32_t hyp_cap,
                                       int32_t* hyp_len, double* score, double* score_lm, double* p_blk, double* p_nblk, int32_t* nbeam) {
    return ctc_beam_host("cn_ctc_merged_beam_host", false,
                         ctc_search_args(ctc_beam_args(logp, top_idx, size_ratio, B, Tp, V, beam, pruning, blank, length_penalty,
                                                       ctc_beam_out(hyp, hyp_cap, hyp_len, score, score_lm, p_blk, p_nblk, nbeam)),
                                         ngram_desc, lm_scale, bias_desc, true));
}

// ---- forced alignment ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_viterbi_kernel(ViterbiArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int S = 2 * a.ymax + 1, Tp = a.Tp;
    float* al0 = reinterpret_cast<float*>(smem);  // alpha[t]
    float* al1 = al0 + S;                         // alpha[t + 1]
    float* alx = al1 + S;                         // alpha[src_size]
    int* path = reinterpret_cast<int*>(alx + S);  // [S] blank-augmented labels
    const float* logp = a.logp + (long long)b * Tp * a.V;
    const unsigned char* km = a.keymask + (long long)b * Tp;
    unsigned char* bp = a.bp + (long long)b * Tp * S;  // state index minus predecessor index: 0, 1 or 2
    int* out = a.out_path + (long long)b * Tp;
    const int ylen = a.label_len[b];
    const int plen = 2 * ylen + 1;
    const int xb = (int)(long long)(a.size_ratio[b] * (float)Tp);
    const float LZ = -1e10f;
    for (int s2 = tid; s2 < S; s2 += 256) {
        const int u = s2 >> 1;
        path[s2] = (s2 & 1) ? (u < a.ymax ? a.labels[(long long)b * a.ld + u] : a.blank) : a.blank;
        if (u >= ylen && (s2 & 1)) path[s2] = a.blank;  // (the reference pads ys with zeros = blank)
        al0[s2] = s2 == 0 ? 0.f : LZ;
    }
    __syncthreads();
    if (xb == 0)
        for (int s2 = tid; s2 < S; s2 += 256) alx[s2] = al0[s2];
    for (int t = 0; t < Tp; ++t) {
        const bool ok = km[t] != 0;
        for (int s2 = tid; s2 < S; s2 += 256) {
            const float m0 = al0[s2];
            const float m1 = s2 >= 1 ? al0[s2 - 1] : LZ;
            float m2 = s2 >= 2 ? al0[s2 - 2] : LZ;
            if (s2 >= 2 && path[s2 - 2] == path[s2]) m2 = LZ;  // blank and repeated labels have two predecessors only
            float mx = m0;
            int ix = 0;
            if (m1 > mx) {
                mx = m1;
                ix = 1;
            }
            if (m2 > mx) {
                mx = m2;
                ix = 2;
            }
            if (s2 >= plen) mx = LZ;
            bp[(long long)t * S + s2] = (unsigned char)ix;
            const float lp = ok ? logp[(long long)t * a.V + path[s2]] : LZ;
            al1[s2] = mx + lp;
        }
        __syncthreads();
        for (int s2 = tid; s2 < S; s2 += 256) {
            al0[s2] = al1[s2];
            if (t + 1 == xb) alx[s2] = al1[s2];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int t = 0; t < Tp; ++t) out[t] = a.blank;
        if (xb >= 0 && xb <= Tp) {
            const int i1 = plen - 1, i2 = plen - 2 >= 0 ? plen - 2 : S - 1;  // (python index -1 wraps to the last state)
            int cur = alx[i1] > alx[i2] ? i1 : i2;
            // src_size 0: aligned[b, -1] is the LAST frame (python index -1 wraps) and the back-trace has no step; alx = alpha[0]
            out[xb >= 1 ? xb - 1 : Tp - 1] = path[cur];
            for (int t = xb - 1; t >= 1; --t) {
                cur = cur - (int)bp[(long long)t * S + cur];
                if (cur < 0) cur += S;
                out[t - 1] = path[cur];
            }
        }
    }
}

int launch_ctc_viterbi(const ViterbiArgs& a, hipStream_t s) {
    if (a.B <= 0) return 0;
    const int S = 2 * a.ymax + 1;
    const size_t lds = (size_t)S * 16 + 64;
    if (a.ymax < 1 || lds > 96 * 1024) {
        cn_set_error("ctc_viterbi: label length out of range");
        return -1;
    }
    static CnAttrOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        CN_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_viterbi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_once.mark(attr_dev);
    }
    hipLaunchKernelGGL(ctc_viterbi_kernel, dim3(a.B), dim3(256), lds, s, a);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}
