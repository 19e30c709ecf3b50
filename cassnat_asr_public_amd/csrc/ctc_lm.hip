// CTC prefix beam search with the TransformerLM fused into the frame loop (src/utils/beam_decode.py:8-93 with lm_model and
// args.ctc_lm_weight > 0) for gfx950: the kernels around the LM step of cn_ctc_beam_lm (model.hip).
//
// The LM-free search (ctc_beam.hip) holds its whole frame loop in one launch.  With the LM in the loop every processed frame
// needs an LM step over the kept hypotheses, so the loop is queued by the host, one iteration per processed frame, and nothing
// returns to the host inside it:
//   schedule   which frames an utterance processes (t <= src_size and blank probability <= 0.95) is known once ctc_out exists:
//              frames[b][k] = its k-th processed frame, count[b] their number.  Iteration k handles frame frames[b][k] of every
//              utterance with k < count[b]; the others are skipped inside the kernels.
//   LM step    over all S = B * beam slots with a position per row (ast.hip: launch_ast_embed_rows / launch_ast_gather_attn_rows)
//   rows       the LM's next-token log-probability row of every slot, double buffered: a hypothesis that did not change ("stay")
//              copies its parent's row, an extended one takes the fresh log-softmax of this iteration's LM step
//   frame      one workgroup per utterance, one thread per candidate: one frame of the shared search (ctc_search.h) with score_lm
//   finish     unrolls the back-pointers (ctc_search.h)
//
// score_lm is the reference's: a Python float that is NOT reset between the candidates of a hypothesis - the j-th non-blank
// candidate carries the parent's score_lm plus double(lm_prob[c_i]) * double(lm_weight) summed over the non-blank labels
// c_1 .. c_j of the pruned list, added one after the other in that order.
//
// LM cache addressing.  A K/V row is addressed by (iteration, slot): the LM step of iteration k writes the row k * S + s of
// slot s if the slot holds a fresh hypothesis, and no other launch ever writes that row.  Every slot carries a table of row
// ids, one per position of its prefix, copied from its parent and extended by the one new id when a label is appended.  So a
// row is written once and never rewritten, however slots are reoccupied: a shorter hypothesis that takes over a slot and later
// grows to a length the slot held before gets rows of later iterations, and the cousins that still reference the old row read
// what they always read.  Cost: iterations x S rows per layer.
#include "kernels.h"

// one thread per utterance: the search's frame predicate, frame by frame
__global__ void ctc_lm_schedule_kernel(const float* __restrict__ logp, const float* __restrict__ size_ratio, int B, int Tp, int V,
                                       int blank, int* __restrict__ frames, int* __restrict__ count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int ssz = cs_src_size(size_ratio[b], Tp);
    int n = 0;
    for (int t = 0; t < Tp && t <= ssz; ++t) {
        if (cs_skip_frame(logp[((long long)b * Tp + t) * V + blank])) continue;
        frames[(long long)b * Tp + n++] = t;
    }
    count[b] = n;
}

// batch_top_seqs = [[{'ys': [[sos]], 'p_blk': logone, 'p_nblk': logzero, 'score_ctc': 0.0, 'score_lm': 0.0, 'hyp': []}]]; the first LM
// step runs on [sos] in every slot (each appends row 0 * S + s of its own, so no slot reads a row nobody wrote)
__global__ void ctc_lm_init_kernel(CtcLmState st, int B, int W, int Lt, int sos) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B * W) return;
    const int j = s % W;
    st.pb[s] = j == 0 ? 0.0 : CS_LOGZERO;
    st.pnb[s] = CS_LOGZERO;
    st.sctc[s] = j == 0 ? 0.0 : CS_LOGZERO;
    st.slm[s] = 0.0;
    st.len[s] = 0;
    st.last[s] = -1;
    st.tok[s] = sos;
    st.pos[s] = 0;
    st.parent[s] = s;
    st.stay[s] = 0;
    st.rowid[0][(long long)s * Lt] = s;
    st.rowid[1][(long long)s * Lt] = s;
    if (j == 0) st.nb[s / W] = 1;
}

// rows of the next frame step: nxt[s] = stay[s] ? prv[parent[s]] : fresh[s]; utterances past their last frame are skipped
__global__ __launch_bounds__(256) void ctc_lm_rows_kernel(const float* __restrict__ fresh, const float* __restrict__ prv,
                                                          float* __restrict__ nxt, const int* __restrict__ parent,
                                                          const int* __restrict__ stay, const int* __restrict__ count, int iter, int W,
                                                          int V) {
    const int s = blockIdx.x;
    if (count && iter >= count[s / W]) return;
    const float* src = stay[s] ? prv + (long long)parent[s] * V : fresh + (long long)s * V;
    float* dst = nxt + (long long)s * V;
    if ((V & 3) == 0) {
        for (int i = threadIdx.x; i < V / 4; i += 256) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < V; i += 256) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(256) void ctc_lm_frame_kernel(CtcLmState st, CtcLmFrame a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W = a.W, P = a.P, NC = W * (P + 1), Lt = a.Lt, S = a.B * W;
    const int s0 = b * W;
    if (a.iter >= a.count[b]) {  // the utterance has no frame left: its beam stands, its slots ask nothing of the LM step
        if (tid < W) st.stay[s0 + tid] = 1;
        return;
    }
    double* pb = reinterpret_cast<double*>(smem);  // [W] state of the kept hypotheses
    double* pnb = pb + W;
    double* pslm = pnb + W;
    double* ckey = pslm + W;  // [NC] candidates
    double* cpb = ckey + NC;
    double* cpnb = cpb + NC;
    double* ctot = cpnb + NC;
    double* cslm = ctot + NC;
    int* blen = reinterpret_cast<int*>(cslm + NC);  // [W]
    int* blast = blen + W;
    int* npar = blast + W;  // [W] parent slot of the new beam's entries (-1: unused)
    int* next = npar + W;   // [W] 1: the entry appended a label
    int* cpar = next + W;   // [NC] parent slot (-1: not a candidate)
    int* ctok = cpar + NC;  // [NC] appended label (-1: stay)
    __shared__ int s_valid;

    const int nb = min(st.nb[b], W), t = a.frames[(long long)b * a.Tp + a.iter];  // (never more candidates than the LDS holds)
    if (t < 0 || t >= a.Tp) return;
    const float* row = a.logp + ((long long)b * a.Tp + t) * a.V;
    const int* top = a.top_idx + ((long long)b * a.Tp + t) * P;
    const int cur = a.iter & 1, nxt = cur ^ 1;
    if (tid < W) {
        pb[tid] = st.pb[s0 + tid];
        pnb[tid] = st.pnb[s0 + tid];
        pslm[tid] = st.slm[s0 + tid];
        blen[tid] = st.len[s0 + tid];
        blast[tid] = st.last[s0 + tid];
        npar[tid] = -1;
        next[tid] = 0;
    }
    __syncthreads();
    const int ncand = nb * (P + 1);
    for (int i = tid; i < ncand; i += 256) {
        const int k = i / (P + 1), j = i - k * (P + 1);
        // (an id outside the vocabulary is no candidate: nothing is read through it)
        const CsCand r = cs_candidate(row, a.V, a.blank, k, j == 0, j == 0 ? -1 : top[j - 1], pb[k], pnb[k], blast[k], blen[k]);
        double slm = pslm[k];  // blank or repetition: the parent's score_lm
        if (r.tok >= 0) {
            // score_lm += lm_prob[s_idx, c].item() * lm_weight over the non-blank labels up to this one, in list order
            const float* lm = a.lmrow + (long long)(s0 + k) * a.V;
            for (int jj = 0; jj < j; ++jj) {
                const int cc = top[jj];
                if (cc != a.blank && cc >= 0 && cc < a.V) slm += cn_mul_rn((double)lm[cc], a.lm_weight);
            }
        }
        cpar[i] = r.par;
        ctok[i] = r.tok;
        cpb[i] = r.pb;
        cpnb[i] = r.pnb;
        ctot[i] = r.tot;
        cslm[i] = slm;
        ckey[i] = cs_key(r.tot, slm, a.lp, r.len);
    }
    __syncthreads();
    // The state of the kept hypotheses is in LDS, so the winners write the new state over it in global memory
    for (int i = tid; i < ncand; i += 256) {
        if (cpar[i] < 0) continue;
        const int rank = cs_rank(ckey, cpar, ncand, i);
        if (rank < W) {
            const int k = cpar[i], tok = ctok[i], sn = s0 + rank;
            const int nlen = blen[k] + (tok >= 0 ? 1 : 0), nlast = tok >= 0 ? tok : blast[k];
            st.pb[sn] = cpb[i];
            st.pnb[sn] = cpnb[i];
            st.sctc[sn] = ctot[i];
            st.slm[sn] = cslm[i];
            st.len[sn] = nlen;
            st.last[sn] = nlast;
            st.tok[sn] = nlast >= 0 ? nlast : a.sos;
            st.pos[sn] = nlen;
            st.parent[sn] = s0 + k;
            st.stay[sn] = tok < 0;
            a.hist_parent[((long long)b * a.hist_stride + a.iter) * W + rank] = (unsigned char)k;
            a.hist_tok[((long long)b * a.hist_stride + a.iter) * W + rank] = tok;
            npar[rank] = k;
            next[rank] = tok >= 0;
        }
    }
    if (tid == 0) s_valid = cs_count_valid(cpar, ncand, W);
    __syncthreads();
    const int nbn = s_valid;
    if (tid == 0) st.nb[b] = nbn;
    if (tid >= nbn && tid < W) {  // an unused slot: a carried dummy
        const int sn = s0 + tid;
        st.tok[sn] = a.sos;
        st.pos[sn] = 0;
        st.parent[sn] = sn;
        st.stay[sn] = 1;
    }
    // row-id tables of the next LM step: the parent's ids, plus row (iter + 1) * S + slot for an appended label
    for (int r = 0; r < nbn; ++r) {
        const int k = npar[r], plen = blen[k];
        const int* src = st.rowid[cur] + (long long)(s0 + k) * Lt;
        int* dst = st.rowid[nxt] + (long long)(s0 + r) * Lt;
        for (int i = tid; i <= plen; i += 256) dst[i] = src[i];
        if (tid == 0 && next[r]) dst[plen + 1] = (a.iter + 1) * S + s0 + r;
    }
}

// one thread per slot: a kept hypothesis unrolls its back-pointers
__global__ void ctc_lm_finish_kernel(CtcLmState st, CtcBeamOut o, const int* __restrict__ count, const unsigned char* __restrict__ hist_parent,
                                     const int* __restrict__ hist_tok, int hist_stride, int W) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid >= W) return;
    const int nb = st.nb[b], s = b * W + tid;
    if (tid == 0) o.n_out[b] = nb;
    CsKept kept = {};
    if (tid < nb) kept = CsKept{st.sctc[s], st.slm[s], st.pb[s], st.pnb[s], st.len[s]};
    cs_write_row(o, s, hist_parent, hist_tok, (long long)b * hist_stride * W, W, count[b], tid < nb ? tid : -1, kept);
}

int launch_ctc_lm_schedule(const float* logp, const float* size_ratio, int B, int Tp, int V, int blank, int* frames, int* count,
                           hipStream_t s) {
    if (B < 1 || Tp < 1 || V < 1 || blank < 0 || blank >= V) {
        cn_set_error("ctc_lm_schedule: need B, T', V >= 1 and the blank inside the vocabulary");
        return -1;
    }
    hipLaunchKernelGGL(ctc_lm_schedule_kernel, dim3(cn_ceil_div(B, 64)), dim3(64), 0, s, logp, size_ratio, B, Tp, V, blank, frames, count);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ctc_lm_init(const CtcLmState& st, int B, int W, int Lt, int sos, hipStream_t s) {
    if (B < 1 || W < 1 || W > 32 || Lt < 1) {
        cn_set_error("ctc_lm_init: need B >= 1, 1 <= ctc_beam <= 32 and a row-id table of at least one entry");
        return -1;
    }
    hipLaunchKernelGGL(ctc_lm_init_kernel, dim3(cn_ceil_div(B * W, 64)), dim3(64), 0, s, st, B, W, Lt, sos);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ctc_lm_rows(const float* fresh, const float* prv, float* nxt, const int* parent, const int* stay, const int* count, int iter,
                       int slots, int W, int V, hipStream_t s) {
    if (slots < 1 || W < 1 || slots % W || V < 1 || iter < 0) {
        cn_set_error("ctc_lm_rows: need slots = B * ctc_beam >= 1, V >= 1 and iteration >= 0");
        return -1;
    }
    hipLaunchKernelGGL(ctc_lm_rows_kernel, dim3(slots), dim3(256), 0, s, fresh, prv, nxt, parent, stay, count, iter, W, V);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ctc_lm_frame(const CtcLmState& st, const CtcLmFrame& a, hipStream_t s) {
    if (a.B <= 0) return 0;
    if (const char* bad = cs_check_limits(a.W, a.P, 0, 0)) {
        cn_set_error(std::string("ctc_lm_frame: ") + bad);
        return -1;
    }
    // (a hypothesis has at most iter labels before this step: ids 0 .. iter + 1 are written)
    if (a.iter < 0 || a.iter >= a.hist_stride || a.Lt < a.iter + 2 || a.Tp < 1 || a.iter >= a.Tp || a.blank < 0 || a.blank >= a.V) {
        cn_set_error("ctc_lm_frame: iteration outside the history / row-id tables, or the blank outside the vocabulary");
        return -1;
    }
    hipLaunchKernelGGL(ctc_lm_frame_kernel, dim3(a.B), dim3(256), cs_lds_bytes(a.W, a.P, true, 4, 2), s, st, a);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ctc_lm_finish(const CtcLmState& st, const CtcBeamOut& o, const int* count, const unsigned char* hist_parent, const int* hist_tok,
                         int hist_stride, int B, int W, hipStream_t s) {
    if (B < 1 || W < 1 || W > 32 || o.Lmax < 1) {
        cn_set_error("ctc_lm_finish: need B >= 1, 1 <= ctc_beam <= 32 and room for a label");
        return -1;
    }
    hipLaunchKernelGGL(ctc_lm_finish_kernel, dim3(B), dim3(64), 0, s, st, o, count, hist_parent, hist_tok, hist_stride, W);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}
