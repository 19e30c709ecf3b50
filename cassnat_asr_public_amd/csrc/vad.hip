// The energy VAD of bin/make_segments on the device: per-frame integer energies of staged int16 audio, and Kaldi's
// compute-vad-decision rule over them.  vad_frames.h holds the arithmetic (the same functions the serial host twins run),
// include/cassnat_hip_vad.h the contract, DESIGN.md 7p the definition.
//
//   frame_energy_kernel  bandwidth-bound: every sample is needed by ceil(N / shift) frames and is read from HBM once.  A workgroup of
//                        256 owns `F` consecutive frames of one row (F = 64 unless their span does not fit the LDS: vf_block_frames,
//                        chosen on the host) and brings the span (F - 1) shift + N sample frames, all channels, into LDS: the 16-byte
//                        pieces from the 16-byte boundary at or below the block's first byte (inside the row when rows start on
//                        multiples of 16, as the contract asks; a piece that starts in front of the row is not loaded whole) up to the
//                        last whole piece that ends inside the span, head and tail as 2-byte loads - no byte outside [row start, end
//                        of the row's clamped samples) is read.  Each wave then takes a quarter of the block's
//                        frames from LDS, two at a time: lanes stride over a frame's samples, S1 in int32, S2 in 64 bits, a butterfly
//                        across the wave; lane j keeps the wave's j-th num, and at the end the lanes form e side by side and do two
//                        ordinary, contiguous vector stores.  No atomics, no scratch memory.
//   vad_partial_kernel   (part, recording): the sum of e over the part's contiguous strip of frames - lanes stride, a butterfly, the four
//                        waves' sums added in order; the same bits in every run.
//   vad_threshold_kernel one thread per recording adds the VF_PARTS partial sums from the first to the last: thr.
//   vad_vote_kernel      (block, recording), workgroups stride over the frames: dec[t] from e[t - context .. t + context] (read again,
//                        through L2) against thr.
// All counts are clamped before they bound a loop and are uniform over a workgroup, so every barrier is reached by all of it.
#include "vad_frames.h"

#include "../../include/cassnat_hip_vad.h"

__global__ __launch_bounds__(VF_THREADS) void frame_energy_kernel(const unsigned char* __restrict__ staged, long long staged_bytes,
                                                                  const int* __restrict__ off, const int* __restrict__ samples,
                                                                  const int* __restrict__ out_off, int N, int shift, int channels, int channel,
                                                                  int remove_dc, int max_frames, int F, long long* __restrict__ num,
                                                                  double* __restrict__ e) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vf_lds[];
    const int r = blockIdx.y, tid = threadIdx.x;
    const long long o = off[r];
    const int n = vf_row_samples(o, samples[r], channels, staged_bytes);
    const int T = vf_num_frames(n, N, shift, max_frames);
    const long long t0 = (long long)blockIdx.x * F;
    if (t0 >= T) return;  // (uniform over the workgroup)
    const int fc = (T - t0) < F ? (int)(T - t0) : F;
    // the block's bytes [b0, b1) lie inside the row's clamped samples: b1 <= o + n * channels * 2 <= staged_bytes
    const long long b0 = o + t0 * shift * channels * 2;
    const long long b1 = b0 + ((long long)(fc - 1) * shift + N) * channels * 2;
    // LDS mirrors the bytes from the 16-byte boundary a0 at or below b0.  Pieces of 16 bytes that lie inside [o, b1) are loaded whole;
    // a first piece that starts in front of the row (a row at an offset that is no multiple of 16) and the bytes behind the last whole
    // piece are loaded as int16 values, so no byte outside [o, b1) is read.
    const long long a0 = b0 & ~15LL;
    const int head = (int)(b0 - a0);
    const int full = (int)((b1 - a0) >> 4);
    const int skip = a0 < o ? 1 : 0;
    const long long hb = skip ? (a0 + 16 < b1 ? a0 + 16 : b1) : b0;  // the int16 head is [b0, hb)
    const long long whole = a0 + 16LL * full;
    const long long tb = whole > hb ? whole : hb;                     // the int16 tail is [tb, b1)
    const uint4* src = reinterpret_cast<const uint4*>(staged + a0);
    uint4* dst = reinterpret_cast<uint4*>(vf_lds);
    short* lds16 = reinterpret_cast<short*>(vf_lds);
    for (int i = tid + skip; i < full; i += VF_THREADS) dst[i] = src[i];
    if (tid < (int)(hb - b0) >> 1) lds16[(head >> 1) + tid] = reinterpret_cast<const short*>(staged + b0)[tid];
    if (tid < (int)(b1 - tb) >> 1) lds16[(int)((tb - a0) >> 1) + tid] = reinterpret_cast<const short*>(staged + tb)[tid];
    __syncthreads();
    // wave w owns the frames [w q, (w + 1) q) of the block, q = ceil(fc / 4) <= 16, two at a time (two independent chains of LDS reads
    // and butterflies in flight); after the butterfly every lane holds the frame's sums, and lane j keeps frame j's num - so the
    // logarithms of a wave's frames are taken side by side and its stores are contiguous
    const int wave = tid >> 6, lane = tid & 63;
    const int q = (fc + VF_THREADS / 64 - 1) / (VF_THREADS / 64);
    const int f0 = wave * q, f1 = f0 + q < fc ? f0 + q : fc;
    const short* base = lds16 + (head >> 1) + channel;
    long long mine = 0;
    for (int f = f0; f < f1; f += 2) {
        const short* xa = base + f * shift * channels;
        const short* xb = base + (f + 1 < f1 ? f + 1 : f) * shift * channels;  // (an odd count: the last frame twice, kept once)
        int S1a = 0, S1b = 0;
        unsigned long long S2a = 0, S2b = 0;
        for (int i = lane; i < N; i += 64) {
            const int va = xa[i * channels], vb = xb[i * channels];
            S1a += va, S1b += vb;
            S2a += (unsigned)(va * va), S2b += (unsigned)(vb * vb);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            S1a += __shfl_xor(S1a, d), S1b += __shfl_xor(S1b, d);
            S2a += __shfl_xor(S2a, d), S2b += __shfl_xor(S2b, d);
        }
        if (lane == f - f0) mine = vf_num(S1a, (long long)S2a, N, remove_dc);
        if (lane == f + 1 - f0) mine = vf_num(S1b, (long long)S2b, N, remove_dc);
    }
    if (lane < f1 - f0) {
        const long long at = (long long)out_off[r] + t0 + f0 + lane;
        num[at] = mine;
        e[at] = vf_log_energy(mine, N, remove_dc);
    }
}

__global__ __launch_bounds__(VF_THREADS) void vad_partial_kernel(const double* __restrict__ e, const int* __restrict__ rec_off,
                                                                 const int* __restrict__ rec_frames, double* __restrict__ parts) {
    __shared__ double wsum[VF_THREADS / 64];
    const int i = blockIdx.y, p = blockIdx.x, tid = threadIdx.x;
    const int T = rec_frames[i] < 0 ? 0 : rec_frames[i];
    const long long L = ((long long)T + VF_PARTS - 1) / VF_PARTS;
    const long long lo = p * L, hi = lo + L < T ? lo + L : T;
    const double* x = e + rec_off[i];
    double s = 0.0;
    for (long long t = lo + tid; t < hi; t += VF_THREADS) s += x[t];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) parts[(long long)i * VF_PARTS + p] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(64) void vad_threshold_kernel(const int* __restrict__ rec_frames, int recs, double thr0, double mean_scale,
                                                           const double* __restrict__ parts, double* __restrict__ thr) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= recs) return;
    double sum = 0.0;
    for (int p = 0; p < VF_PARTS; ++p) sum += parts[(long long)i * VF_PARTS + p];
    thr[i] = vf_threshold(thr0, mean_scale, sum, rec_frames[i]);
}

__global__ __launch_bounds__(VF_THREADS) void vad_vote_kernel(const double* __restrict__ e, const int* __restrict__ rec_off,
                                                              const int* __restrict__ rec_frames, int context, double proportion,
                                                              const double* __restrict__ thr, unsigned char* __restrict__ dec) {
    const int i = blockIdx.y;
    const int T = rec_frames[i] < 0 ? 0 : rec_frames[i];
    const double* x = e + rec_off[i];
    unsigned char* d = dec + rec_off[i];
    const double th = thr[i];
    for (long long t = (long long)blockIdx.x * VF_THREADS + threadIdx.x; t < T; t += (long long)gridDim.x * VF_THREADS)
        d[t] = (unsigned char)vf_vote(x, T, (int)t, context, th, proportion);
}

static int vf_refuse(const char* who, const char* why) {
    if (!why) return 0;
    cn_set_error(std::string(who) + ": " + why);
    return -1;
}

extern "C" int cn_op_frame_energy(const void* staged_dev, int64_t staged_bytes, const int32_t* off_dev, const int32_t* samples_dev,
                                  const int32_t* out_off_dev, int32_t rows, int32_t N, int32_t shift, int32_t channels, int32_t channel,
                                  int32_t remove_dc, int32_t max_frames, int64_t* num_dev, double* e_dev, void* stream) {
    CN_TRY(vf_refuse("cn_op_frame_energy", vf_check_energy(staged_dev, off_dev, samples_dev, out_off_dev, num_dev, e_dev, rows, N, shift, channels,
                                                           channel, max_frames)));
    if (staged_bytes < 0 || ((size_t)staged_dev & 15)) return vf_refuse("cn_op_frame_energy", "the staged bytes must start on a 16-byte boundary");
    const int F = vf_block_frames(N, shift, channels);
    const long long blocks = ((long long)max_frames + F - 1) / F;
    hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(VF_THREADS), (size_t)vf_block_bytes(F, N, shift, channels),
                       (hipStream_t)stream, static_cast<const unsigned char*>(staged_dev), (long long)staged_bytes, off_dev, samples_dev, out_off_dev,
                       N, shift, channels, channel, remove_dc ? 1 : 0, max_frames, F, reinterpret_cast<long long*>(num_dev), e_dev);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cn_frame_energy_host(const void* staged, int64_t staged_bytes, const int32_t* off, const int32_t* samples, const int32_t* out_off,
                                    int32_t rows, int32_t N, int32_t shift, int32_t channels, int32_t channel, int32_t remove_dc,
                                    int32_t max_frames, int64_t* num, double* e) {
    CN_TRY(vf_refuse("cn_frame_energy_host", vf_check_energy(staged, off, samples, out_off, num, e, rows, N, shift, channels, channel, max_frames)));
    if (staged_bytes < 0) return vf_refuse("cn_frame_energy_host", "staged_bytes < 0");
    vf_frame_energy_host(static_cast<const uint8_t*>(staged), staged_bytes, off, samples, out_off, rows, N, shift, channels, channel,
                         remove_dc ? 1 : 0, max_frames, num, e);
    return 0;
}

extern "C" int cn_op_vad_decide(const double* e_dev, const int32_t* rec_off_dev, const int32_t* rec_frames_dev, int32_t recs, double thr0,
                                double mean_scale, int32_t context, double proportion, double* thr_dev, uint8_t* dec_dev, void* stream) {
    CN_TRY(vf_refuse("cn_op_vad_decide", vf_check_decide(e_dev, rec_off_dev, rec_frames_dev, thr_dev, dec_dev, recs, context)));
    hipStream_t s = (hipStream_t)stream;
    double* parts = thr_dev + recs;
    hipLaunchKernelGGL(vad_partial_kernel, dim3(VF_PARTS, (unsigned)recs), dim3(VF_THREADS), 0, s, e_dev, rec_off_dev, rec_frames_dev, parts);
    CN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(vad_threshold_kernel, dim3((unsigned)cn_ceil_div(recs, 64)), dim3(64), 0, s, rec_frames_dev, recs, thr0, mean_scale, parts,
                       thr_dev);
    CN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(vad_vote_kernel, dim3(VF_PARTS, (unsigned)recs), dim3(VF_THREADS), 0, s, e_dev, rec_off_dev, rec_frames_dev, context,
                       proportion, thr_dev, dec_dev);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cn_vad_decide_host(const double* e, const int32_t* rec_off, const int32_t* rec_frames, int32_t recs, double thr0, double mean_scale,
                                  int32_t context, double proportion, double* thr, uint8_t* dec) {
    CN_TRY(vf_refuse("cn_vad_decide_host", vf_check_decide(e, rec_off, rec_frames, thr, dec, recs, context)));
    vf_decide_host(e, rec_off, rec_frames, recs, thr0, mean_scale, context, proportion, thr, dec);
    return 0;
}
