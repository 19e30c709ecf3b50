// Kernels of the CASS-NAT finish loop with LM shallow fusion (src/models/cassnat.py:574-637 with args.lm_weight > 0) on the
// device.  The decode pass left the decoder's log-probability rows att_out [B][U][V]; step i of the loop adds
// lm_weight * lm_model(ys, mask)[:, -1] to row i of every live hypothesis before the top-k.  Hypothesis slot s = b * bw + j is
// also its slot in the TransformerLM's step cache (as in ast.hip): the LM step runs on every slot at every step, a fused row
// kernel gives every slot its bw best continuations, and one workgroup per utterance ranks the bw * bw candidates and writes
// the next beam with the ancestor / key-mask tables the next LM step gathers through.  Nothing returns to the host inside
// the loop: utterance b consumes steps 0 .. last[b] = min(ylen[b], ymax - 1), which the host knows before it starts.
#include "beam_core.h"
#include "rowreduce.h"

// local_prob = att_prob + lm_weight * lm_prob; torch.topk(local_prob, beam_width) (cassnat.py:606-611).  One workgroup per
// slot.  The attention operand is row (b, step) of the engine's LOG-PROBABILITY rows - it is not normalised again (what
// logsoftmax_topk_kernel<true> does to its first operand) - or an all-zero row for a step at or past zlen[b] (ESA: att_out
// masked by the selected sample's own length, cassnat.py:536).  The LM operand is the slot's row of raw logits: its maximum
// and log-sum-exp by rowreduce.h, as in logsoftmax_topk_kernel / logsoftmax_gather_kernel, then every entry becomes
// att + fl32(w * ((x - max) - lse)), float32 with one rounding per operation (no FMA contraction), and k rounds select on that
// sum (sorted descending, ties: lower index first).  A selected entry is retired with a NaN, which is never chosen again: a row
// with fewer than k entries above -inf (an -inf LM logit of an overflowing half-precision engine) yields its -inf entries one
// by one, lower index first, as torch.topk would - never an index twice.
__global__ __launch_bounds__(256) void nat_lm_fuse_topk_kernel(NatFuseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* row = reinterpret_cast<float*>(smem);
    __shared__ RowReduceLds red;
    const int slot = blockIdx.x, b = slot / a.bw;
    // the utterance has ended: its beams are carried, nothing reads this slot's row (the whole workgroup leaves, before any barrier)
    if (a.last && a.step > a.last[b]) return;
    const int tid = threadIdx.x, V = a.V;
    const float* pl = a.lm + (long long)slot * V;
    const bool zero = a.zlen && a.step >= a.zlen[b];
    const float* pa = a.att + ((long long)b * a.U + a.step) * V;
    float lbest = -INFINITY;
    for (int i = tid; i < V; i += 256) {
        const float v = pl[i];
        row[i] = v;
        lbest = fmaxf(lbest, v);
    }
    const float lmax = rr_block_max(red, tid, lbest);
    const float llse = rr_block_lse(red, row, V, tid, lmax);
    for (int i = tid; i < V; i += 256)
        row[i] = __fadd_rn(zero ? 0.f : pa[i], cn_mul_rn(a.w, __fsub_rn(__fsub_rn(row[i], lmax), llse)));
    rr_select_rounds(red, row, V, tid, a.k, __builtin_nanf(""), [&](int r, int bidx, float best) {
        // (a row of NaNs has no winner: token 0 then, never an index outside the vocabulary - it becomes an embedding row)
        a.idx[(long long)slot * a.k + r] = bidx < V ? bidx : 0;
        a.val[(long long)slot * a.k + r] = best;
    });
}

int launch_nat_lm_fuse_topk(const NatFuseArgs& a, int slots, hipStream_t s) {
    if (a.k < 1 || a.k > 32 || a.k > a.V || a.V > 8192 || a.bw < 1 || a.U < 1 || a.step < 0 || a.step >= a.U) {
        cn_set_error("nat_lm_fuse_topk: need 1 <= k <= min(32, V), V <= 8192, beam_width >= 1 and 0 <= step < rows per utterance");
        return -1;
    }
    if (slots <= 0) return 0;
    hipLaunchKernelGGL(nat_lm_fuse_topk_kernel, dim3(slots), dim3(256), (size_t)a.V * sizeof(float), s, a);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// batch_top_seqs = [[{'ys': [[sos]], 'score': 0.0, 'hyp': [sos]}]] (cassnat.py:574-578), both parities; last[b] = the last
// step utterance b consumes (the loop reads row i while i <= ylen[b], i < ymax); every final hypothesis of b has last[b] + 2 tokens
__global__ void nat_beam_init_kernel(NatBeamState st, const int* __restrict__ ylen, int ymax, int* __restrict__ last,
                                     int* __restrict__ hyp_len, int B, int bw, int L, int sos, int pad) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B * bw) return;
    const int b = s / bw;
    for (int p = 0; p < 2; ++p) beam_init_row(st, p, s, L, sos, pad);
    st.cur_tok[s] = sos;
    const int l = ylen[b] < ymax - 1 ? ylen[b] : ymax - 1;
    if (s == b * bw) last[b] = l;
    if (hyp_len) hyp_len[s] = l + 2;
}

constexpr int NAT_MAXW = 16, NAT_MAXC = NAT_MAXW * NAT_MAXW;

// One step of the beam bookkeeping (cassnat.py:613-636), one workgroup per utterance, one thread per candidate.  Live beams:
// one at step 0, bw afterwards (every beam brings bw candidates, so the list never runs short).  Candidates beam by beam, j
// ascending; score = parent score (double) + (double)value; key = score + (len(hyp) - 1) * length_penalty in double (every
// candidate of a step has step + 2 tokens) or the score alone; ties keep list order (Python's stable sort).
__global__ __launch_bounds__(NAT_MAXC) void nat_beam_update_kernel(NatBeamState st, NatBeamStep q) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int bw = q.bw, L = q.L, cur = q.cur, nxt = cur ^ 1;
    __shared__ double ckey[NAT_MAXC], cscore[NAT_MAXC];
    __shared__ int ctok[NAT_MAXC], newslot[NAT_MAXW];
    if (q.step > q.last[b]) {  // past the utterance's rows: its beams are carried unchanged (cassnat.py:587-589)
        for (int i = tid; i < bw * L; i += NAT_MAXC) {
            const long long o = (long long)b * bw * L + i;
            st.tok[nxt][o] = st.tok[cur][o];
            st.anc[nxt][o] = st.anc[cur][o];
            st.keyok[nxt][o] = st.keyok[cur][o];
        }
        if (tid < bw) st.score[nxt][b * bw + tid] = st.score[cur][b * bw + tid];
        return;
    }
    const int nl = q.step == 0 ? 1 : bw, ncand = nl * bw;
    if (tid < NAT_MAXW) newslot[tid] = 0;  // (NaN keys rank nowhere: every slot still names a candidate of this utterance)
    __syncthreads();
    if (tid < ncand) {
        const int s = b * bw + tid / bw;
        const long long c = (long long)s * bw + (tid - (tid / bw) * bw);
        const double sc = st.score[cur][s] + (double)q.val[c];
        cscore[tid] = sc;
        ckey[tid] = beam_key(sc, q.step + 1, q.lp, q.use_lp);
        ctok[tid] = q.idx[c];
    }
    __syncthreads();
    if (tid < ncand) {
        const int r = beam_rank(ckey, ncand, tid);
        if (r < bw) newslot[r] = tid;
    }
    __syncthreads();
    for (int qn = 0; qn < bw; ++qn) {
        const int e = newslot[qn];
        const int so = b * bw + e / bw, sn = b * bw + qn;
        beam_write_row(st, cur, L, so, sn, true, q.step + 1, q.step, ctok[e], q.pad, tid, NAT_MAXC);  // (every candidate grows)
        if (tid == 0) {
            st.score[nxt][sn] = cscore[e];
            st.cur_tok[sn] = ctok[e];
        }
    }
}

int launch_nat_beam_init(const NatBeamState& st, const int* ylen, int ymax, int* last, int* hyp_len, int B, int bw, int L, int sos,
                         int pad, hipStream_t s) {
    if (B < 1 || bw < 1 || bw > NAT_MAXW || ymax < 1 || L < ymax + 1) {
        cn_set_error("nat beam: need B >= 1, 1 <= beam_width <= 16, ymax >= 1 and max_len >= ymax + 1");
        return -1;
    }
    hipLaunchKernelGGL(nat_beam_init_kernel, dim3(cn_ceil_div(B * bw, 64)), dim3(64), 0, s, st, ylen, ymax, last, hyp_len, B, bw, L, sos,
                       pad);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_nat_beam_update(const NatBeamState& st, const NatBeamStep& q, int B, hipStream_t s) {
    // (step + 1 is the position the update writes: it must lie inside the L tokens of a slot)
    if (B < 1 || q.bw < 1 || q.bw > NAT_MAXW || q.step < 0 || q.L < q.step + 2 || (q.cur != 0 && q.cur != 1)) {
        cn_set_error("nat beam: need B >= 1, 1 <= beam_width <= 16, 0 <= step <= max_len - 2 and cur 0 or 1");
        return -1;
    }
    hipLaunchKernelGGL(nat_beam_update_kernel, dim3(B), dim3(NAT_MAXC), 0, s, st, q);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}
