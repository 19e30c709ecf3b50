// CTC prefix beam search with word n-gram fusion for gfx950: `decode_type: ctc_only / ctc_att` with `rank_model: n-gram`, an ARPA
// model and ctc_lm_weight > 0.  The reference has no such search (its in-loop fusion is the TransformerLM's, ctc_lm.hip); this one is
// ctc_beam_decode's search (ctc_beam.hip) with score_lm = lm_scale * (the word scores of the words a hypothesis has closed), the words
// being the ones the n-gram ranker's gluing finds (ngram.hip).  ctc_ngram_search.h holds the semantics and the step functions; the
// serial host search there and the kernel here are made of the same functions.
//
// ctc_ngram_beam_kernel is laid out like ctc_prefix_beam_kernel: one workgroup of 256 per utterance, the frame loop inside, one
// candidate per thread (in rounds when there are more than 256), the stable top-W by counting rank, (parent, label) back-pointers per
// processed frame, unrolled at the end.  On top of that:
//   * the n-gram state of the kept hypotheses (CgHyp: carry, history, word count, score_lm and the cached value of closing the open
//     word) lives in LDS in two buffers: a winner writes slot `rank` of the other buffer from its parent's slot of this one;
//   * what closing a word adds depends on the parent alone, so table look-ups are per kept hypothesis whose open word changed (at most
//     W a frame), not per candidate: the winner's thread finds the word's id, then the up to 2 * order - 1 probes of the word's score
//     are spread over (hypothesis, task) threads and one thread per hypothesis adds them up in ng_word_score's float32 order;
//   * after the last frame every kept hypothesis adds its open word and </s>, and the beam is sorted once more by the same key.
// Every probe loop is bounded by its table's slot count; labels outside [0, V) make no candidate.
#include "ctc_ngram_search.h"
#include "kernels.h"

// the word scores of hypotheses r < n with flag[r] set, word wid[r] behind hy[r]'s history: probes by (hypothesis, task) threads, then
// thread r returns double(score) * lm_scale (0 for the others).  All 256 threads call it; the caller puts a barrier behind its use.
__device__ __forceinline__ double cg_score_words(const cn_ngram_desc& d, const CgHyp* hy, const int* flag, const int* wid, int n,
                                                 NgProbe* probes, double lm_scale) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n * CG_TASKS; i += 256) {
        const int r = i / CG_TASKS, t = i - r * CG_TASKS;
        if (t < CG_TASKS - 1 && flag[r]) cg_probe(d, hy[r].hist + NG_HIST, cg_context(d, hy[r]), wid[r], t, &probes[i]);
    }
    __syncthreads();
    if (tid < n && flag[tid]) return (double)cg_word_score(probes + tid * CG_TASKS, cg_context(d, hy[tid])) * lm_scale;
    return 0.0;
}

__global__ __launch_bounds__(256) void ctc_ngram_beam_kernel(CtcNgramArgs a) {
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
    double* cslm = ctot + NC;
    double* ptot = cslm + NC;                      // [W] score_ctc of the kept hypotheses
    int* blen = reinterpret_cast<int*>(ptot + W);  // [W]
    int* blast = blen + W;                         // [W] last label (-1: empty hypothesis)
    int* cpar = blast + W;                         // [NC] parent slot (-1: not a candidate)
    int* ctok = cpar + NC;                         // [NC] appended label (-1: stay)
    int* clen = ctok + NC;
    int* clast = clen + NC;
    __shared__ CgHyp hyps[2][CG_MAX_BEAM];  // n-gram state, double buffered
    __shared__ NgProbe probes[CG_MAX_BEAM * CG_TASKS];
    __shared__ int wflag[CG_MAX_BEAM], wid[CG_MAX_BEAM], frank[CG_MAX_BEAM];
    __shared__ int s_nb, s_steps;

    const cn_ngram_desc& d = a.d;
    const float* logp = a.logp + (long long)b * a.Tp * a.V;
    const int* top = a.top_idx + (long long)b * a.Tp * P;
    unsigned char* hpar = a.hist_parent + (long long)b * a.Tp * W;
    int* htok = a.hist_tok + (long long)b * a.Tp * W;
    const int ssz = cg_src_size(a.size_ratio[b], a.Tp);
    if (tid == 0) {
        pb[0] = 0.0;  // logone
        pnb[0] = CG_LOGZERO;
        ptot[0] = 0.0;
        blen[0] = 0;
        blast[0] = -1;
        cg_init(d, &hyps[0][0]);
        s_nb = 1;
        s_steps = 0;
    }
    int cur = 0;
    __syncthreads();
    for (int t = 0; t < a.Tp; ++t) {
        if (t > ssz) continue;  // (the reference does process frame t == src_size)
        const float* row = logp + (long long)t * a.V;
        if (cg_skip_frame(row[a.blank])) continue;
        const int nb = s_nb, step = s_steps;
        const int ncand = nb * (P + 1);
        for (int i = tid; i < ncand; i += 256) {
            const int k = i / (P + 1), j = i - k * (P + 1);
            const int c = j == 0 ? -1 : top[(long long)t * P + (j - 1)];
            const CgCand r = cg_candidate(d, row, a.V, a.blank, k, j == 0, c, pb[k], pnb[k], blast[k], blen[k], hyps[cur][k], a.lp);
            cpar[i] = r.par;
            ctok[i] = r.tok;
            clen[i] = r.len;
            clast[i] = r.last;
            cpb[i] = r.pb;
            cpnb[i] = r.pnb;
            ctot[i] = r.tot;
            cslm[i] = r.slm;
            ckey[i] = r.key;
        }
        if (tid < W) wflag[tid] = 0;
        __syncthreads();
        // stable descending order: rank = candidates that sort before this one
        for (int i = tid; i < ncand; i += 256) {
            if (cpar[i] < 0) continue;
            const double key = ckey[i];
            int rank = 0;
            for (int j = 0; j < ncand; ++j) {
                if (cpar[j] < 0) continue;
                const double kj = ckey[j];
                rank += (kj > key || (kj == key && j < i)) ? 1 : 0;
            }
            if (rank < W) {
                pb[rank] = cpb[i];
                pnb[rank] = cpnb[i];
                ptot[rank] = ctot[i];
                blen[rank] = clen[i];
                blast[rank] = clast[i];
                hpar[(long long)step * W + rank] = (unsigned char)cpar[i];
                htok[(long long)step * W + rank] = ctok[i];
                CgHyp* h = &hyps[cur ^ 1][rank];
                if (cg_advance(d, hyps[cur][cpar[i]], ctok[i], h) && h->carry.pw != 1) {
                    wid[rank] = h->close_wid = ng_word_id(d, h->carry.h);
                    wflag[rank] = 1;
                }
            }
        }
        // (pb / pnb / blen / blast were only read in the candidate phase above, behind the barrier: safe to overwrite)
        if (tid == 0) {
            int valid = 0;
            for (int j = 0; j < ncand; ++j) valid += cpar[j] >= 0 ? 1 : 0;
            s_nb = valid < W ? valid : W;
            s_steps = step + 1;
        }
        __syncthreads();
        cur ^= 1;
        const int kept = s_nb;
        const double add = cg_score_words(d, hyps[cur], wflag, wid, kept, probes, a.lm_scale);
        if (tid < kept && wflag[tid]) hyps[cur][tid].close_add = add;
        __syncthreads();
    }
    // the open word, then </s>, and one more stable sort by the same key
    const int nb = s_nb, steps = s_steps;
    if (tid < nb) {
        CgHyp* h = &hyps[cur][tid];
        if (h->carry.pw != 1) cg_push_word(h, h->close_wid, h->close_add);
        wflag[tid] = 1;
        wid[tid] = d.eos;
    }
    __syncthreads();
    const double add = cg_score_words(d, hyps[cur], wflag, wid, nb, probes, a.lm_scale);
    if (tid < nb) {
        hyps[cur][tid].slm += add;
        ckey[tid] = (ptot[tid] + hyps[cur][tid].slm) + a.lp * (double)blen[tid];
    }
    __syncthreads();
    if (tid < nb) {
        const double key = ckey[tid];
        int rank = 0;
        for (int j = 0; j < nb; ++j) rank += (ckey[j] > key || (ckey[j] == key && j < tid)) ? 1 : 0;
        frank[tid] = rank;
    }
    // unroll the back-pointers: one thread per kept hypothesis, written at its final rank
    if (tid == 0) a.n_out[b] = nb;
    if (tid < W) {
        const int out = tid < nb ? frank[tid] : tid;
        int* h = a.hyp + ((long long)b * W + out) * a.Lmax;
        const long long o = (long long)b * W + out;
        if (tid < nb) {
            const int len = blen[tid];
            int pos = len - 1, at = tid;
            for (int st = steps - 1; st >= 0; --st) {
                const int tok = htok[(long long)st * W + at];
                if (tok >= 0) {
                    if (pos >= 0 && pos < a.Lmax) h[pos] = tok;
                    --pos;
                }
                at = hpar[(long long)st * W + at];
            }
            for (int i = len < 0 ? 0 : len; i < a.Lmax; ++i) h[i] = 0;
            a.hyp_len[o] = len;
            a.score[o] = ptot[tid];
            a.score_lm[o] = hyps[cur][tid].slm;
            a.p_blk[o] = pb[tid];
            a.p_nblk[o] = pnb[tid];
        } else {
            for (int i = 0; i < a.Lmax; ++i) h[i] = 0;
            a.hyp_len[o] = 0;
            a.score[o] = CG_LOGZERO;
            a.score_lm[o] = 0.0;
            a.p_blk[o] = CG_LOGZERO;
            a.p_nblk[o] = CG_LOGZERO;
        }
    }
}

int launch_ctc_ngram_beam(const CtcNgramArgs& a, hipStream_t s) {
    const std::string bad = cg_check(a, true);
    if (!bad.empty()) {
        cn_set_error("ctc_ngram_beam: " + bad);
        return -1;
    }
    const int NC = a.W * (a.P + 1);
    const size_t lds = (size_t)(3 * a.W + 5 * NC) * 8 + (size_t)(2 * a.W + 4 * NC) * 4 + 64;
    static CnAttrOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        CN_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_ngram_beam_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_once.mark(attr_dev);
    }
    hipLaunchKernelGGL(ctc_ngram_beam_kernel, dim3(a.B), dim3(256), lds, s, a);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// the same search on the host: every pointer a host pointer, no GPU call
extern "C" int cn_ctc_ngram_beam_host(const cn_ngram_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                                      int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, double lm_scale,
                                      int32_t blank, int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm,
                                      double* p_blk, double* p_nblk, int32_t* nbeam) {
    if (!desc) {
        cn_set_error("cn_ctc_ngram_beam_host: null argument");
        return -1;
    }
    CtcNgramArgs a;
    a.d = *desc;
    a.logp = logp, a.top_idx = top_idx, a.size_ratio = size_ratio;
    a.B = B, a.Tp = Tp, a.V = V, a.P = pruning, a.W = beam, a.blank = blank, a.Lmax = hyp_cap;
    a.lp = length_penalty, a.lm_scale = lm_scale;
    a.hyp = hyp, a.hyp_len = hyp_len, a.score = score, a.score_lm = score_lm, a.p_blk = p_blk, a.p_nblk = p_nblk, a.n_out = nbeam;
    const std::string bad = cg_check(a, false);
    if (!bad.empty()) {
        cn_set_error("cn_ctc_ngram_beam_host: " + bad);
        return -1;
    }
    for (int32_t b = 0; b < B; ++b) cg_search_host(a, b);
    return 0;
}
