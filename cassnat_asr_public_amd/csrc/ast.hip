// Kernels of the autoregressive (AST) decoder step with a KV cache - BASELINE config 4, SURVEY 8a row a18.
// Reference: Transformer.beam_decode (src/models/transformer.py:122-241) re-runs the whole decoder on the full prefix
// at every step; here only the NEW position of every live hypothesis is computed and the keys/values of the earlier
// positions are read from a cache.
//
// Cache layout: K and V of decoder layer l, position j, written by the hypothesis that occupied row ("slot") s of the live
// list at step j:  cache[l][j][s][d].  Every (j, s) cell is written exactly once (at step j), so a hypothesis never copies
// its parent's cache: it carries an ancestor table anc[j] = slot that wrote position j of its prefix, and the attention
// kernel gathers through it.  HBM-bound gather work - no MFMA (one query row per hypothesis).
#include "beam_core.h"

// x[h][:] = lut[tok[h]][:] * sqrt(d) + pe[pos][:]        (TextEmbedding + PositionalEncoding, embedding.py:71-78, 29-31)
__global__ void ast_embed_kernel(const int* __restrict__ tok, const float* __restrict__ lut, const float* __restrict__ pe_row,
                                 float* __restrict__ x, int n, int d, float scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * d) return;
    const int h = i / d, c = i - h * d;
    x[i] = lut[(long long)tok[h] * d + c] * scale + pe_row[c];
}

int launch_ast_embed(const int* tok, const float* lut, const float* pe_row, float* x, int n, int d, float scale,
                     hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ast_embed_kernel, dim3(cn_ceil_div(n * d, 256)), dim3(256), 0, s, tok, lut, pe_row, x, n, d, scale);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Single-query multi-head attention with gathered key/value rows (d_k = 64).  One workgroup per row of queries, one wave per
// head.  Phase 1: a lane owns a key (64-dim dot product with the query held in registers); masked keys get float-min
// exactly like MultiHeadedAttention (attention.py:19-21).  Phase 2: a lane owns an output dimension.
// One body, ga_head, does the work of a (row, head) wave.  The forms differ in the keys of a row, which a key set describes:
//   n           keys of the row: j in [0, n)
//   ld          row length of k / v, in elements
//   row(j)      the row of k / v that holds key j
//   allowed(j)  false: the key scores float-min
//   own         the key whose K | V are still in the projection buffer (columns d.. and 2d.. of q's row), or < 0 for none: the
//               wave writes its 64 columns of them to row own_row of k / v for the steps to come and reads key `own` from the
//               projection buffer itself (no separate append launch, no read-after-write through the cache)
// ---------------------------------------------------------------------------------------------
// decoder self-attention over the KV cache [pos][slots][d]: key j is cache row (j, anc[j]), allowed iff keyok[j]
struct GaCacheKeys {
    const int* anc;              // the row's [table_stride] entries
    const unsigned char* keyok;  // the row's [table_stride] entries
    int slots, n, ld, own;
    long long own_row;
    __device__ long long row(int j) const { return (long long)j * slots + anc[j]; }
    __device__ bool allowed(int j) const { return keyok[j] != 0; }
};
// source attention over the fused K | V matrix [B * n][2d]: key j is row first + j, allowed iff the utterance's keymask[j]
struct GaSourceKeys {
    const unsigned char* keymask;  // the utterance's [n] entries
    long long first;
    int n, ld;
    static constexpr int own = -1;
    static constexpr long long own_row = 0;
    __device__ long long row(int j) const { return first + j; }
    __device__ bool allowed(int j) const { return keymask[j] != 0; }
};
// a position per row (ctc_lm.hip): key j is the absolute cache row ids[j], every key allowed (a CTC hypothesis holds no padding)
struct GaRowKeys {
    const int* ids;  // the row's [table_stride] entries
    int n, ld, own;
    long long own_row;
    __device__ long long row(int j) const { return ids[j]; }
    __device__ bool allowed(int) const { return true; }
};

// bytes per element of a row of T (a split-bf16 pair is 4); head hd of a row is 64 consecutive columns = 64 * ES contiguous bytes
// in every layout
template <typename T> constexpr int ga_elem_bytes = __is_same(T, split_t) ? 4 : (int)sizeof(T);

// sc: the wave's n scores in LDS
template <typename T, typename Keys>
__device__ __forceinline__ void ga_head(const Keys& ks, const void* q_base, int ldq, int d, const void* k_base, const void* v_base,
                                        void* o_base, int ldo, float scale, float* sc) {
    const int h = blockIdx.x, lane = threadIdx.x & 63, hd = threadIdx.x >> 6;
    constexpr int ES = ga_elem_bytes<T>;
    const unsigned char* qrow = reinterpret_cast<const unsigned char*>(q_base) + ((long long)h * ldq + hd * 64) * ES;
    float q[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) q[i] = cn_ld_row_elem<T>(qrow, i);
    const bool append = ks.own >= 0;
    const unsigned char* new_k = qrow + (long long)d * ES;  // (head hd of this row's K | V in the fused projection)
    const unsigned char* new_v = qrow + (long long)2 * d * ES;
    const unsigned char* kb = reinterpret_cast<const unsigned char*>(k_base);
    const unsigned char* vb = reinterpret_cast<const unsigned char*>(v_base);
    if (append) {  // the head's 64 * ES bytes of K and of V, ES bytes per lane (a byte copy: any element layout)
        const long long crow = (ks.own_row * ks.ld + hd * 64) * ES + lane * ES;
        if constexpr (ES == 4) {
            *reinterpret_cast<unsigned*>(const_cast<unsigned char*>(kb) + crow) = *reinterpret_cast<const unsigned*>(new_k + lane * 4);
            *reinterpret_cast<unsigned*>(const_cast<unsigned char*>(vb) + crow) = *reinterpret_cast<const unsigned*>(new_v + lane * 4);
        } else {
            *reinterpret_cast<unsigned short*>(const_cast<unsigned char*>(kb) + crow) = *reinterpret_cast<const unsigned short*>(new_k + lane * 2);
            *reinterpret_cast<unsigned short*>(const_cast<unsigned char*>(vb) + crow) = *reinterpret_cast<const unsigned short*>(new_v + lane * 2);
        }
    }
    float lmax = -INFINITY;
    for (int j = lane; j < ks.n; j += 64) {
        const unsigned char* kr = (append && j == ks.own) ? new_k : kb + (ks.row(j) * ks.ld + hd * 64) * ES;
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < 64; ++i) dot = fmaf(q[i], cn_ld_row_elem<T>(kr, i), dot);
        const float s = ks.allowed(j) ? dot * scale : CN_NEG_FILL;
        sc[j] = s;
        lmax = fmaxf(lmax, s);
    }
    lmax = wave_max(lmax);
    float lsum = 0.f;
    for (int j = lane; j < ks.n; j += 64) {
        const float e = expf(sc[j] - lmax);
        sc[j] = e;
        lsum += e;
    }
    lsum = wave_sum(lsum);
    __builtin_amdgcn_wave_barrier();
    // phase 2: lane = output dimension; LDS writes above are visible to the whole wave (same wave, program order)
    const float inv = 1.f / lsum;
    float acc = 0.f;
    for (int j = 0; j < ks.n; ++j) {
        const unsigned char* vr = (append && j == ks.own) ? new_v : vb + (ks.row(j) * ks.ld + hd * 64) * ES;
        acc = fmaf(sc[j], cn_ld_row_elem<T>(vr, lane), acc);
    }
    cn_st_row_elem<T>(reinterpret_cast<unsigned char*>(o_base) + ((long long)h * ldo + hd * 64) * ES, lane, acc * inv);
}

//   MODE 0 (self, cache):  key j in [0, nkeys): row (j*slots + anc[h][j]) of ck / cv (row length d), allowed iff keyok[h][j];
//                          append_pos >= 0: the row's own key, appended to cache row (append_pos, slot h)
//   MODE 1 (source):       key j in [0, nkeys): row (utt[h]*nkeys + j) of the fused K|V matrix (row length 2d), allowed iff
//                          keymask[utt[h]][j]
template <typename T, int MODE>
__global__ void ast_gather_attn_kernel(GatherAttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int h = blockIdx.x, hd = threadIdx.x >> 6;
    float* sc = reinterpret_cast<float*>(smem) + (long long)hd * p.nkeys;
    if constexpr (MODE == 0) {
        const long long t = (long long)h * p.table_stride;
        const GaCacheKeys ks{p.anc + t, p.keyok + t, p.slots, p.nkeys, p.d, p.append_pos, (long long)p.append_pos * p.slots + h};
        ga_head<T>(ks, p.q, p.ldq, p.d, p.k, p.v, p.o, p.ldo, p.scale, sc);
    } else {
        const long long first = (long long)p.utt[h] * p.nkeys;
        const GaSourceKeys ks{p.keymask + first, first, p.nkeys, 2 * p.d};
        ga_head<T>(ks, p.q, p.ldq, p.d, p.k, p.v, p.o, p.ldo, p.scale, sc);
    }
}

// launch(element type tag) for the rows of a precision: fp32, split-bf16 (strides in whole groups of 32 elements) or the 16-bit type
template <typename Launch>
static int ga_for_precision(int prec, const char* who, int ldq, int ldo, int d, Launch launch) {
    if (prec == CN_PREC_F32) {
        launch(float{});
    } else if (prec == CN_PREC_X3) {
        if (ldq % 32 || ldo % 32 || d % 32) {
            cn_set_error(std::string(who) + ": split-bf16 rows need strides that are multiples of 32 elements");
            return -1;
        }
        launch(split_t{});
    } else {
        launch(bf16{});
    }
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ast_gather_attn(int prec, int mode, const GatherAttnArgs& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (a.H < 1 || a.H > 16 || a.nkeys < 1) {
        cn_set_error("ast_gather_attn: need 1 <= heads <= 16 and at least one key");
        return -1;
    }
    GatherAttnArgs p = a;
    if (mode != 0) p.append_pos = -1;
    const size_t lds = (size_t)a.H * a.nkeys * sizeof(float);
    if (lds > 64 * 1024) {
        cn_set_error("ast_gather_attn: too many keys for the score buffer");
        return -1;
    }
    const dim3 grid(a.n), block(64 * a.H);
    return ga_for_precision(prec, "ast_gather_attn", a.ldq, a.ldo, a.d, [&](auto tag) {
        using T = decltype(tag);
        if (mode == 0) hipLaunchKernelGGL((ast_gather_attn_kernel<T, 0>), grid, block, lds, s, p);
        else hipLaunchKernelGGL((ast_gather_attn_kernel<T, 1>), grid, block, lds, s, p);
    });
}

// ---------------------------------------------------------------------------------------------
// The same two kernels with a position PER ROW (ctc_lm.hip: the hypotheses of a CTC prefix beam have different lengths).
//   embed:     x[h][:] = lut[tok[h]][:] * sqrt(d) + pe[pos[h]][:]
//   attention: row h has pos[h] + 1 keys; key j is cache row rowid[h][j] (an absolute row of ck / cv, row length d), every key
//              allowed.  stay[h] == 0: the row's own key is pos[h], appended to cache row rowid[h][pos[h]], as MODE 0 does with
//              append_pos.  stay[h] != 0: the hypothesis did not change - its LM row is carried by the caller - so the
//              workgroup appends nothing and writes a zero context row (rows are independent in everything downstream).
// ---------------------------------------------------------------------------------------------
__global__ void ast_embed_rows_kernel(const int* __restrict__ tok, const float* __restrict__ lut, const float* __restrict__ pe,
                                      const int* __restrict__ pos, float* __restrict__ x, int n, int d, float scale, int max_pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * d) return;
    const int h = i / d, c = i - h * d;
    const int q = pos[h] < 0 ? 0 : (pos[h] > max_pos ? max_pos : pos[h]);  // (a position outside the table reads its last row, never past it)
    x[i] = lut[(long long)tok[h] * d + c] * scale + pe[(long long)q * d + c];
}

int launch_ast_embed_rows(const int* tok, const float* lut, const float* pe, const int* pos, float* x, int n, int d, float scale,
                          int max_pos, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ast_embed_rows_kernel, dim3(cn_ceil_div(n * d, 256)), dim3(256), 0, s, tok, lut, pe, pos, x, n, d, scale, max_pos);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
__global__ void ast_gather_attn_rows_kernel(GatherRowsArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int h = blockIdx.x, lane = threadIdx.x & 63, hd = threadIdx.x >> 6;
    const int apos = p.pos[h];
    if (p.stay[h] || apos < 0 || apos >= p.max_keys) {  // (a position outside the score buffer: nothing is read or written through it)
        cn_st_row_elem<T>(reinterpret_cast<unsigned char*>(p.o) + ((long long)h * p.ldo + hd * 64) * ga_elem_bytes<T>, lane, 0.f);
        return;
    }
    const int* ids = p.rowid + (long long)h * p.table_stride;
    const GaRowKeys ks{ids, apos + 1, p.d, apos, ids[apos]};
    ga_head<T>(ks, p.q, p.ldq, p.d, p.k, p.v, p.o, p.ldo, p.scale, reinterpret_cast<float*>(smem) + (long long)hd * p.max_keys);
}

int launch_ast_gather_attn_rows(int prec, const GatherRowsArgs& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (a.H < 1 || a.H > 16 || a.max_keys < 1 || a.table_stride < a.max_keys || !a.rowid || !a.pos || !a.stay) {
        cn_set_error("ast_gather_attn_rows: need 1 <= heads <= 16, 1 <= max_keys <= table_stride and the row tables");
        return -1;
    }
    const size_t lds = (size_t)a.H * a.max_keys * sizeof(float);
    if (lds > 64 * 1024) {
        cn_set_error("ast_gather_attn_rows: too many keys for the score buffer");
        return -1;
    }
    const dim3 grid(a.n), block(64 * a.H);
    return ga_for_precision(prec, "ast_gather_attn_rows", a.ldq, a.ldo, a.d, [&](auto tag) {
        hipLaunchKernelGGL((ast_gather_attn_rows_kernel<decltype(tag)>), grid, block, lds, s, a);
    });
}

// ---------------------------------------------------------------------------------------------
// CTC side of joint decoding (src/models/transformer.py:135-141, src/utils/ctc_prefix.py).
// ---------------------------------------------------------------------------------------------
#define CN_LOGZERO (-1e10f)

// ctc_out.masked_fill_(src_mask^T == 0, logzero); ctc_out[:, :, blank].masked_fill_(src_mask == 0, 0)
__global__ void ast_ctc_mask_kernel(float* __restrict__ logp, const unsigned char* __restrict__ keymask, int rows, int V,
                                    int blank) {
    const int r = blockIdx.x;
    if (r >= rows || keymask[r]) return;
    float* p = logp + (long long)r * V;
    for (int i = threadIdx.x; i < V; i += blockDim.x) p[i] = i == blank ? 0.f : CN_LOGZERO;
}

// CTCPrefixScore.initial_state: r0[b][t] = (logzero, cumsum_t x[b][t][blank])   (sequential fp32 sum, as torch.cumsum)
__global__ void ast_ctc_init_kernel(const float* __restrict__ logp, float* __restrict__ r0, int B, int Tp, int V, int blank) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float run = 0.f;
    for (int t = 0; t < Tp; ++t) {
        run += logp[((long long)b * Tp + t) * V + blank];
        r0[((long long)b * Tp + t) * 2 + 0] = CN_LOGZERO;
        r0[((long long)b * Tp + t) * 2 + 1] = run;
    }
}

int launch_ast_ctc_prepare(float* logp, const unsigned char* keymask, float* r0, int B, int Tp, int V, int blank,
                           hipStream_t s) {
    hipLaunchKernelGGL(ast_ctc_mask_kernel, dim3(B * Tp), dim3(256), 0, s, logp, keymask, B * Tp, V, blank);
    hipLaunchKernelGGL(ast_ctc_init_kernel, dim3(cn_ceil_div(B, 64)), dim3(64), 0, s, logp, r0, B, Tp, V, blank);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

__device__ __forceinline__ float lse2(float a, float b) {  // torch.logsumexp over two values
    const float m = fmaxf(a, b);
    return m + logf(expf(a - m) + expf(b - m));
}

// CTCPrefixScore.__call__ (ctc_prefix.py:50-106): one thread per (hypothesis, candidate label), sequential over frames.
__global__ void ast_ctc_prefix_kernel(CtcPrefixArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n * a.K) return;
    const int h = i / a.K;
    const int c = a.cand[i];
    const int u = a.utt[h];
    const int Tp = a.Tp;
    const float* x = a.logp + (long long)u * Tp * a.V;
    const int ref = a.prev_ref[h];
    const float* rp = ref < 0 ? a.r0 + (long long)(-1 - ref) * Tp * 2 : a.r_prev + (long long)ref * Tp * 2;
    float* r = a.r_new + (long long)i * Tp * 2;
    const bool same = a.last_tok[h] == c;
    const int L = a.out_len;
    const int start = L > 1 ? L : 1;
    for (int t = 0; t < start; ++t) {
        r[2 * t] = CN_LOGZERO;
        r[2 * t + 1] = CN_LOGZERO;
    }
    if (L == 0) r[0] = x[c];
    // log_phi(t) = last(g) == c ? r_prev^b(t) : logsumexp(r_prev^n(t), r_prev^b(t))
    float rn = r[2 * (start - 1)], rb = r[2 * (start - 1) + 1];
    // log_psi = logsumexp over { r^n(start-1) } U { log_phi(t-1) + x_c(t), t in [start, T) }: streaming max/sum
    float pm = rn, ps = 1.f;
    // The recurrence is sequential in t, its inputs are not: the loads of 8 frames go out together (the one-frame-at-a-time
    // loop spent 0.7 us per frame waiting for them), then the 8 updates run in the reference's order.
    for (int t0 = start; t0 < Tp; t0 += 8) {
        float2 pv[8];
        float xcv[8], xbv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = t0 + j < Tp ? t0 + j : Tp - 1;
            pv[j] = *reinterpret_cast<const float2*>(rp + 2 * (t - 1));
            xcv[j] = x[(long long)t * a.V + c];
            xbv[j] = x[(long long)t * a.V + a.blank];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = t0 + j;
            if (t < Tp) {
                const float p0 = pv[j].x, p1 = pv[j].y;
                const float phi = same ? p1 : lse2(p0, p1);
                const float xc = xcv[j], xb = xbv[j];
                const float nn = lse2(rn, phi) + xc;
                const float nb = lse2(rn, rb) + xb;
                *reinterpret_cast<float2*>(r + 2 * t) = make_float2(nn, nb);
                rn = nn;
                rb = nb;
                const float v = phi + xc;
                if (v > pm) {
                    ps = ps * expf(pm - v) + 1.f;
                    pm = v;
                } else {
                    ps += expf(v - pm);
                }
            }
        }
    }
    float psi = pm + logf(ps);
    if (c == a.eos) psi = lse2(rp[2 * (Tp - 1)], rp[2 * (Tp - 1) + 1]);
    if (c == a.blank) psi = CN_LOGZERO;
    a.score[i] = psi;
}

int launch_ast_ctc_prefix(const CtcPrefixArgs& a, hipStream_t s) {
    // out_len > Tp: the first loop would write states past the candidate's Tp x 2 block (the reference raises IndexError there)
    if (a.Tp < 1 || a.out_len < 0 || a.out_len > a.Tp) {
        cn_set_error("ast_ctc_prefix: need 0 <= out_len <= Tp (a hypothesis longer than the CTC frames)");
        return -1;
    }
    if (a.n <= 0 || a.K <= 0) return 0;
    hipLaunchKernelGGL(ast_ctc_prefix_kernel, dim3(cn_ceil_div(a.n * a.K, 64)), dim3(64), 0, s, a);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Device-side beam bookkeeping of Transformer.beam_decode (src/models/transformer.py:157-240).  Hypothesis slot s =
// b * bw + j is also its KV-cache slot; every slot runs every step (finished / unused ones compute on dummies and are
// ignored), so nothing is compacted and nothing returns to the host inside the loop.  One workgroup per utterance:
// <= bw finished hypotheses are carried, every live hypothesis contributes its top-bw of K candidates (stable order,
// like the host path's stable argsort), all candidates are ranked by score + (len - 1) * length_penalty with ties in
// list order (Python's stable sort), the best bw become the next beam.  Arithmetic follows the reference's types:
// float32 for the per-candidate combination (no FMA contraction), Python-float (double) score accumulation and keys.
// ---------------------------------------------------------------------------------------------------------------
__global__ void ast_beam_init_kernel(AstBeamState st, int cur, int B, int bw, int L, int sos, int pad) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B * bw) return;
    const int b = s / bw, j = s - b * bw;
    beam_init_row(st, cur, s, L, sos, pad);
    st.len[cur][s] = 1;
    st.valid[cur][s] = j == 0;
    st.ctc_ref[cur][s] = -1 - b;
    st.ctc_prev[cur][s] = 0.f;
    st.cur_tok[s] = sos;
    st.utt[s] = b;
    if (s == 0) *st.live = B;
}

// beams and candidate lists up to 32 wide (conf/decode.yaml: beam_width 20, ctc_beam 30): at 32 / 32 the candidate list is 1056
// entries, 38 KB of LDS
constexpr int BEAM_MAXW = 32, BEAM_MAXC = BEAM_MAXW + BEAM_MAXW * BEAM_MAXW, BEAM_THREADS = 256;

__global__ __launch_bounds__(BEAM_THREADS) void ast_beam_update_kernel(AstBeamState st, AstBeamStep q) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int bw = q.bw, K = q.K, L = q.L, cur = q.cur, nxt = cur ^ 1;
    __shared__ double ckey[BEAM_MAXC], cscore[BEAM_MAXC];
    __shared__ int cpar[BEAM_MAXC], ccand[BEAM_MAXC], ctok[BEAM_MAXC], newslot[BEAM_MAXW];
    __shared__ float cctc[BEAM_MAXC], loc[BEAM_MAXW][BEAM_MAXW];
    __shared__ int fin_idx[BEAM_MAXW], live_idx[BEAM_MAXW], nf_s, nl_s;
    if (tid == 0) {
        int nf = 0, nl = 0;
        for (int j = 0; j < bw; ++j) {
            const int s = b * bw + j;
            if (!st.valid[cur][s]) continue;
            const int last = st.tok[cur][(long long)s * L + st.len[cur][s] - 1];
            if (last == q.eos) fin_idx[nf++] = j; else live_idx[nl++] = j;
        }
        nf_s = nf;
        nl_s = nl;
    }
    if (tid < BEAM_MAXW) newslot[tid] = -1;
    __syncthreads();
    const int nf = nf_s, nl = nl_s;
    if (tid < nf) {  // finished hypotheses are carried as they are
        const int s = b * bw + fin_idx[tid];
        const double sc = st.score[cur][s];
        cscore[tid] = sc;
        ckey[tid] = beam_key(sc, st.len[cur][s] - 1, q.lp, q.use_lp);
        cpar[tid] = fin_idx[tid];
        ccand[tid] = -1;
    }
    for (int i = tid; i < nl * K; i += BEAM_THREADS) {
        const int li = i / K, c = i - li * K;
        const int s = b * bw + live_idx[li];
        const float att = q.att[(long long)s * K + c];
        // local = ctc_weight * (ctc - prev) + (1 - ctc_weight) * att, float32, one rounding per operation (transformer.py:205-206)
        // (cn_mul_rn: the products are rounded before the sums - hipcc would otherwise contract them into FMAs)
        float v = q.use_ctc ? __fadd_rn(cn_mul_rn(q.w, __fsub_rn(q.ctc[(long long)s * K + c], st.ctc_prev[cur][s])), cn_mul_rn(q.u, att))
                            : att;
        // local += lm_weight * lm_prob.gather(1, indices) (transformer.py:208-209); without CTC `att` already holds the fused sum
        if (q.use_lm && q.use_ctc) v = __fadd_rn(v, cn_mul_rn(q.lw, q.lm[(long long)s * K + c]));
        loc[li][c] = v;
    }
    __syncthreads();
    for (int i = tid; i < nl * K; i += BEAM_THREADS) {
        const int li = i / K, c = i - li * K;
        const float v = loc[li][c];
        int r = 0;
        for (int c2 = 0; c2 < K; ++c2) r += (loc[li][c2] > v) || (loc[li][c2] == v && c2 < c);
        if (r < bw) {
            const int j = live_idx[li], s = b * bw + j, e = nf + li * bw + r;
            const double sc = st.score[cur][s] + (double)v;
            cscore[e] = sc;
            ckey[e] = beam_key(sc, st.len[cur][s], q.lp, q.use_lp);  // new length - 1 = old length
            cpar[e] = j;
            ccand[e] = c;
            ctok[e] = q.idx[(long long)s * K + c];
            cctc[e] = q.use_ctc ? q.ctc[(long long)s * K + c] : 0.f;
        }
    }
    __syncthreads();
    const int ncand = nf + nl * (K < bw ? K : bw);
    for (int e = tid; e < ncand; e += BEAM_THREADS) {
        const int r = beam_rank(ckey, ncand, e);
        if (r < bw) newslot[r] = e;
    }
    __syncthreads();
    int live_new = 0;
    for (int qn = 0; qn < bw; ++qn) {
        const int e = newslot[qn];
        const int sn = b * bw + qn;
        if (e < 0) {  // fewer candidates than beam slots: an unused slot with harmless inputs for the next step
            for (int t = tid; t < L; t += BEAM_THREADS) st.anc[nxt][(long long)sn * L + t] = sn;
            if (tid == 0) {
                st.valid[nxt][sn] = 0;
                st.len[nxt][sn] = 1;
                st.score[nxt][sn] = 0.0;
                st.ctc_ref[nxt][sn] = -1 - b;
                st.ctc_prev[nxt][sn] = 0.f;
                st.cur_tok[sn] = q.sos;
            }
            continue;
        }
        const int so = b * bw + cpar[e];
        const int len_o = st.len[cur][so];
        const bool grown = ccand[e] >= 0;
        beam_write_row(st, cur, L, so, sn, grown, len_o, q.pos, grown ? ctok[e] : 0, q.pad, tid, BEAM_THREADS);
        if (tid == 0) {
            st.valid[nxt][sn] = 1;
            st.len[nxt][sn] = len_o + (grown ? 1 : 0);
            st.score[nxt][sn] = cscore[e];
            st.ctc_ref[nxt][sn] = grown ? so * K + ccand[e] : st.ctc_ref[cur][so];
            st.ctc_prev[nxt][sn] = grown ? cctc[e] : st.ctc_prev[cur][so];
            st.cur_tok[sn] = grown ? ctok[e] : q.eos;
        }
        live_new += grown && ctok[e] != q.eos;
    }
    if (tid == 0 && live_new) atomicAdd(st.live, live_new);
}

int launch_ast_beam_init(const AstBeamState& st, int cur, int B, int bw, int L, int sos, int pad, hipStream_t s) {
    hipLaunchKernelGGL(ast_beam_init_kernel, dim3(cn_ceil_div(B * bw, 64)), dim3(64), 0, s, st, cur, B, bw, L, sos, pad);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ast_beam_update(const AstBeamState& st, const AstBeamStep& q, int B, hipStream_t s) {
    // (K < bw: the candidate list would have holes - e = nf + li * bw + r, r < K - and torch.topk refuses it too)
    if (q.bw < 1 || q.bw > BEAM_MAXW || q.K < q.bw || q.K > BEAM_MAXW) {
        cn_set_error("ast beam: need 1 <= beam_width <= candidate count <= 32");
        return -1;
    }
    CN_HIP_CHECK(hipMemsetAsync(st.live, 0, sizeof(int), s));
    hipLaunchKernelGGL(ast_beam_update_kernel, dim3(B), dim3(BEAM_THREADS), 0, s, st, q);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}
