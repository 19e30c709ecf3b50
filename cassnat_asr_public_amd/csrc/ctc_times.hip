// CTC token time stamps for gfx950: a forced alignment of given labels with per-token spans and confidences (decode_asr --hip_ctm).
// ctc_times_search.h holds the step functions, include/cassnat_hip_ctc_times.h the contract.  It is not ctc_viterbi_kernel
// (ctc_beam.hip), which restates the reference's float32 viterbi_align for the trigger mask of decode_type ctc_att.
//
// One workgroup of 256 per utterance, everything of the frame loop in LDS:
//   * the two live alpha rows in float64, state s with thread s % 256 (rows wider than the workgroup go round by round);
//   * the emissions logp[t][path[s]] of a block of frames, gathered by all threads at once in front of the block's frames, so the
//     frame loop itself reads no global memory and the gather's latency is paid once per block, not once per frame;
//   * the back-pointers, 2 bits per (frame, state): the wave that owns a chunk of 64 states writes two __ballot masks per frame.  In
//     the scratch form (rows too long for the LDS, or the caller's threshold) the same two words go to global memory instead.
//   One barrier per frame: frame t reads row A and writes row B, frame t + 1 the other way round.
// The walk back is serial by nature: wave 0 follows the masks out of LDS (every lane the same state, the reads broadcast), leaves the
// spans in LDS, and all threads then take a token each: the span's largest log-posterior and the stores.
// Every index is checked first: n and L are clamped, a bad label ends the utterance with status 2 before anything is read through it,
// and every barrier is reached by the whole workgroup (status, n and L are uniform over it).
#include "ctc_times_search.h"
#include "kernels.h"
#include "model.h"

using namespace cn_host;

template <bool BP_LDS>
__global__ __launch_bounds__(CT_THREADS) void ctc_times_kernel(CtcTimesArgs a, int emis_floats, int lds_fixed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_bad, s_rep;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Smax = 2 * a.ld + 1;
    double* prev = reinterpret_cast<double*>(smem);       // [Smax]
    double* next = prev + Smax;                            // [Smax]
    float* emis = reinterpret_cast<float*>(next + Smax);  // [emis_floats]
    int* path = reinterpret_cast<int*>(emis + emis_floats);  // [Smax]
    const int n = ct_clamp(a.frames[b], 0, a.Tp), L = ct_clamp(a.label_len[b], 0, a.ld), S = 2 * L + 1, chunks = ct_chunks(S);
    unsigned long long* bp;
    if constexpr (BP_LDS)
        bp = reinterpret_cast<unsigned long long*>(smem + lds_fixed);
    else
        bp = a.bp + (size_t)b * (a.Tp - 1) * ct_chunks(Smax) * 2;  // (n - 1 <= Tp - 1 rows of chunks <= ct_chunks(Smax))
    const int32_t* lab = a.labels + (size_t)b * a.ld;
    const float* logp = a.logp + (size_t)b * a.Tp * a.V;
    int32_t* start = a.start + (size_t)b * a.ld;
    int32_t* end = a.end + (size_t)b * a.ld;
    float* conf = a.conf + (size_t)b * a.ld;
    const double ninf = -INFINITY;

    if (tid == 0) s_bad = s_rep = 0;
    __syncthreads();
    int bad = 0, rep = 0;
    for (int u = tid; u < L; u += CT_THREADS) {
        const int32_t y = lab[u];
        if (!ct_label_ok(y, a.V, a.blank)) bad = 1;
        if (u > 0 && lab[u - 1] == y) ++rep;
        path[2 * u + 1] = y;
        path[2 * u + 2] = a.blank;
    }
    if (tid == 0) path[0] = a.blank;
    if (bad) atomicOr(&s_bad, 1);
    if (rep) atomicAdd(&s_rep, rep);
    __syncthreads();
    const int status = s_bad ? 2 : (L + s_rep > n ? 1 : 0);
    if (status != 0 || n == 0) {  // (uniform: the whole workgroup leaves; n == 0 with status 0 is the empty path, L == 0)
        for (int u = tid; u < L; u += CT_THREADS) {
            start[u] = end[u] = -1;
            conf[u] = 0.f;
        }
        if (tid == 0) {
            a.status[b] = status;
            a.score[b] = status ? ninf : 0.0;
        }
        return;
    }

    int fb = emis_floats / S;  // frames of an emission block (S <= Smax <= emis_floats)
    if (fb > CT_MAX_FB) fb = CT_MAX_FB;
    for (int t0 = 0; t0 < n; t0 += fb) {
        const int nf = n - t0 < fb ? n - t0 : fb;
        // (a state's label in a register, eight frames' loads in flight per thread before the first of them is stored)
        for (int s = tid; s < S; s += CT_THREADS) {
            const float* col = logp + (size_t)t0 * a.V + path[s];
            for (int f = 0; f < nf; f += 8) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = f + j < nf ? col[(size_t)(f + j) * a.V] : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (f + j < nf) emis[(f + j) * S + s] = v[j];
            }
        }
        __syncthreads();
        for (int f = 0; f < nf; ++f) {
            const int t = t0 + f;
            const float* e = emis + f * S;
            if (t == 0) {
                for (int s = tid; s < S; s += CT_THREADS) next[s] = s < 2 ? (double)e[s] : ninf;
            } else {
                for (int base = 0; base < S; base += CT_THREADS) {  // (uniform over the workgroup: every wave reaches its ballots)
                    const int s = base + tid;
                    int move = 0;
                    if (s < S) {
                        const bool has2 = (s & 1) && s >= 3 && path[s - 2] != path[s];
                        const double mx = ct_step(prev[s], s >= 1 ? prev[s - 1] : 0.0, has2 ? prev[s - 2] : 0.0, s >= 1, has2, &move);
                        next[s] = mx + (double)e[s];
                    }
                    const unsigned long long lo = __ballot(move & 1), hi = __ballot(move & 2);
                    if ((tid & 63) == 0 && s < S) {
                        unsigned long long* w = bp + ((size_t)(t - 1) * chunks + (s >> 6)) * 2;
                        w[0] = lo;
                        w[1] = hi;
                    }
                }
            }
            __syncthreads();
            double* x = prev;
            prev = next;
            next = x;
        }
    }
    // prev: the last frame's row; next is free and holds the spans from here on
    const int cur = ct_end_state(L, L ? prev[2 * L - 1] : 0.0, L ? prev[2 * L] : 0.0);
    const double score = prev[cur];
    int32_t* st = reinterpret_cast<int32_t*>(next);
    int32_t* en = st + L;
    for (int u = tid; u < L; u += CT_THREADS) st[u] = en[u] = -1;
    __syncthreads();
    if (tid < 64) ct_walk(bp, chunks, n, cur, st, en);
    __syncthreads();
    for (int u = tid; u < L; u += CT_THREADS) {
        const int s0 = st[u], e0 = en[u];
        start[u] = s0;
        end[u] = e0;
        conf[u] = ct_conf(logp, a.V, path[2 * u + 1], s0, e0);
    }
    if (tid == 0) {
        a.status[b] = 0;
        a.score[b] = score;
    }
}

template <bool BP_LDS>
static int launch_times(const CtcTimesArgs& a, hipStream_t s) {
    static CnAttrOnce attr_once;  // (one per instantiation)
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        CN_HIP_CHECK(hipFuncSetAttribute((const void*)ctc_times_kernel<BP_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CT_LDS_CAP));
        attr_once.mark(attr_dev);
    }
    const int Smax = 2 * a.ld + 1;
    const size_t fixed = ct_lds_fixed(Smax), lds = fixed + (BP_LDS ? ct_bp_bytes(a.Tp, Smax) : 0);
    hipLaunchKernelGGL(ctc_times_kernel<BP_LDS>, dim3((unsigned)a.B), dim3(CT_THREADS), lds, s, a, ct_emis_floats(Smax), (int)fixed);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_ctc_token_times(const CtcTimesArgs& a, long long bp_lds_limit, hipStream_t s) {
    const std::string bad = ct_check(a);
    if (!bad.empty()) {
        cn_set_error("ctc_token_times: " + bad);
        return -1;
    }
    if (ct_bp_in_lds(a.Tp, a.ld, bp_lds_limit)) return launch_times<true>(a, s);
    if (!a.bp && ct_scratch_bytes(a.B, a.Tp, a.ld, bp_lds_limit) > 0) {
        cn_set_error("ctc_token_times: the scratch form needs its back-pointer buffer");
        return -1;
    }
    return launch_times<false>(a, s);
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
// frames[b] = set key-mask entries of utterance b (one thread per utterance; the rows are short)
__global__ void ctc_times_frames_kernel(const unsigned char* __restrict__ keymask, int B, int Tp, int* __restrict__ frames) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = 0;
    for (int t = 0; t < Tp; ++t) n += keymask[(size_t)b * Tp + t] != 0;
    frames[b] = n;
}

extern "C" int cn_ctc_token_times(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                                  const cn_decode_opts* opts, const int32_t* labels_dev, int32_t ld, const int32_t* label_len_dev,
                                  int32_t* start_dev, int32_t* end_dev, float* conf_dev, double* score_dev, int32_t* status_dev, void* stream) {
    (void)size_ratio_dev;
    // (a NAT model, or the autoregressive model with its CTC head, as ctc_search_open)
    if (m && m->finalized && (!opts || m->cfg.ast == 2 || !m->ctc_gen.W)) {
        cn_set_error("cn_ctc_token_times: needs a model with a CTC head and decode options");
        return -1;
    }
    CN_TRY(check_call(m, B, T, F));
    if (!labels_dev || !label_len_dev || !start_dev || !end_dev || !conf_dev || !score_dev || !status_dev) {
        cn_set_error("cn_ctc_token_times: null argument");
        return -1;
    }
    if (ld < 1 || ld > CT_MAX_LD) {
        cn_set_error("cn_ctc_token_times: the label row width ld must lie in 1 .. " + std::to_string(CT_MAX_LD));
        return -1;
    }
    CtcTimesArgs a;
    a.labels = labels_dev, a.label_len = label_len_dev;
    a.B = B, a.V = m->cfg.vocab_size, a.ld = ld, a.blank = opts->padding_idx;
    a.start = start_dev, a.end = end_dev, a.conf = conf_dev, a.score = score_dev, a.status = status_dev;
    hipStream_t s = (hipStream_t)stream;
    CN_HIP_CHECK(hipSetDevice(m->cfg.device));
    CN_TRY(stage_encode_ctc_rows(m, feats_dev, B, T, F, opts, s));
    const int Tp = m->Tp;
    if (opts->capture) CN_TRY(capture(m, "ctc_out", m->logits, false, CN_DTYPE_F32, {B, Tp, a.V}, s));
    int* frames = nullptr;
    CN_TRY(scratch_buf(m, "ct_frames", (size_t)B * 4, (void**)&frames));
    hipLaunchKernelGGL(ctc_times_frames_kernel, dim3(cn_ceil_div(B, 64)), dim3(64), 0, s, m->keymask, B, Tp, frames);
    CN_HIP_CHECK(hipGetLastError());
    a.logp = m->logits, a.frames = frames, a.Tp = Tp;
    if (const size_t need = ct_scratch_bytes(B, Tp, ld, -1)) CN_TRY(scratch_buf(m, "ct_bp", need, (void**)&a.bp));
    ProfScope ps(m, "ctc_token_times", 0, (double)B * Tp * (2 * ld + 1) * 4, s);
    return launch_ctc_token_times(a, -1, s);
}

// the same step functions on the host: every pointer a host pointer, no GPU call
extern "C" int cn_ctc_token_times_host(const float* logp, const int32_t* frames, const int32_t* labels, int32_t ld, const int32_t* label_len,
                                       int32_t B, int32_t Tp, int32_t V, int32_t blank, int64_t bp_lds_limit, int32_t* start, int32_t* end,
                                       float* conf, double* score, int32_t* status) {
    (void)bp_lds_limit;
    CtcTimesArgs a;
    a.logp = logp, a.frames = frames, a.labels = labels, a.label_len = label_len;
    a.B = B, a.Tp = Tp, a.V = V, a.ld = ld, a.blank = blank;
    a.start = start, a.end = end, a.conf = conf, a.score = score, a.status = status;
    const std::string bad = ct_check(a);
    if (!bad.empty()) {
        cn_set_error("cn_ctc_token_times_host: " + bad);
        return -1;
    }
    for (int32_t b = 0; b < B; ++b) ct_align_host(a, b);
    return 0;
}
