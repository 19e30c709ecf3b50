// The energy voice-activity detector of bin/make_segments (Kaldi's compute-vad-decision rule): the arithmetic the kernels (vad.hip) and
// the serial host twins (cn_frame_energy_host / cn_vad_decide_host; tools/vad_check.cpp builds them with a plain C++ compiler under
// sanitizers) are both made of.  The contract is in include/cassnat_hip_vad.h, the definition in DESIGN.md 7p; tests/vad_model.py
// restates it in Python integers.
//
// The frame energy is INTEGER arithmetic up to one conversion: S1 = sum x (|S1| < 2^27), S2 = sum x^2 (< 2^41), num = N S2 - S1^2 (with
// DC removal; N times the frame's summed squared deviation from its mean, < 2^52) or num = S2, exact in int64 and in double.  Then
// E = double(num) / N (one rounding) or double(num), and e = log(max(E, 2^-23)) - Kaldi's raw log-energy before pre-emphasis and
// window, after DC removal, with dither 0.  Kernel and twin therefore agree in every bit of num; e differs by what two 1-ulp
// logarithms differ.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include "common.h"
#define VF_HD __host__ __device__ __forceinline__
#else
#define VF_HD inline
#endif

constexpr int VF_MAX_N = 2048;         // frame length in samples
constexpr int VF_MAX_CHANNELS = 8;
constexpr int VF_MAX_CONTEXT = 64;
constexpr int VF_THREADS = 256;        // four waves
constexpr int VF_BLOCK_FRAMES = 64;    // frames of one workgroup (fewer when their span does not fit VF_LDS_BYTES)
constexpr int VF_LDS_BYTES = 64 * 1024;
constexpr int VF_PARTS = 64;           // partial sums of the mean per recording (CN_VAD_PARTS of the header)

// ---- frames ------------------------------------------------------------------------------------------------------------------------
// whole sample frames of a row that lie inside [0, staged_bytes): a row whose offset is negative or odd has none (the contract asks
// for multiples of 16; any even offset is read correctly, a sample is never read across two bytes of different parity)
VF_HD int vf_row_samples(long long off, int samples, int channels, long long staged_bytes) {
    if (off < 0 || (off & 1) || samples <= 0 || off >= staged_bytes) return 0;
    const long long inside = (staged_bytes - off) / (2 * channels);
    return samples < inside ? samples : (int)inside;
}
VF_HD int vf_num_frames(int n, int N, int shift, int max_frames) {  // snip-edges
    if (n < N) return 0;
    const int T = 1 + (n - N) / shift;
    return T < max_frames ? T : max_frames;
}
VF_HD long long vf_num(long long S1, long long S2, int N, int remove_dc) { return remove_dc ? (long long)N * S2 - S1 * S1 : S2; }
VF_HD double vf_log_energy(long long num, int N, int remove_dc) {
    const double E = remove_dc ? (double)num / (double)N : (double)num;
    const double floor_e = 1.1920928955078125e-07;  // 2^-23, Kaldi's numeric_limits<float>::epsilon()
    return log(E < floor_e ? floor_e : E);
}
// frames per workgroup: the most, up to VF_BLOCK_FRAMES, whose span (f - 1) shift + N sample frames fits the LDS behind up to 14 bytes
// of head; at least 1 (N channels 2 <= 32 KiB)
inline int vf_block_frames(int N, int shift, int channels) {
    const long long per = (long long)shift * channels * 2, first = (long long)N * channels * 2 + 16;
    const long long f = 1 + (VF_LDS_BYTES - first) / per;
    return f > VF_BLOCK_FRAMES ? VF_BLOCK_FRAMES : (int)f;
}
inline long long vf_block_bytes(int frames, int N, int shift, int channels) {
    return ((((long long)(frames - 1) * shift + N) * channels * 2 + 16) + 15) / 16 * 16;
}

// ---- decision ----------------------------------------------------------------------------------------------------------------------
VF_HD double vf_threshold(double thr0, double mean_scale, double sum, int T) {
#pragma clang fp contract(off)
    if (mean_scale == 0.0 || T <= 0) return thr0;
    const double mean = sum / (double)T;
    const double scaled = mean_scale * mean;
    return thr0 + scaled;
}
VF_HD int vf_vote(const double* e, int T, int t, int context, double thr, double proportion) {
#pragma clang fp contract(off)
    const int lo = t - context < 0 ? 0 : t - context, hi = t + context > T - 1 ? T - 1 : t + context;
    int num = 0;
    for (int k = lo; k <= hi; ++k) num += e[k] > thr;
    const double need = (double)(hi - lo + 1) * proportion;
    return (double)num >= need;
}

// ---- the serial twins ------------------------------------------------------------------------------------------------------------------
inline const char* vf_check_energy(const void* staged, const void* off, const void* samples, const void* out_off, const void* num, const void* e,
                                   int rows, int N, int shift, int channels, int channel, int max_frames) {
    if (!staged || !off || !samples || !out_off || !num || !e) return "null argument";
    if (rows <= 0 || rows > 65535) return "need 1 <= rows <= 65535";
    if (N < 1 || N > VF_MAX_N) return "the frame length N must lie in 1 .. 2048 samples";
    if (shift < 1) return "need shift >= 1";
    if (channels < 1 || channels > VF_MAX_CHANNELS) return "channels must lie in 1 .. 8";
    if (channel < 0 || channel >= channels) return "channel must name one of the channels";
    if (max_frames < 1) return "need max_frames >= 1";
    return nullptr;
}
inline const char* vf_check_decide(const void* e, const void* rec_off, const void* rec_frames, const void* thr, const void* dec, int recs,
                                   int context) {
    if (!e || !rec_off || !rec_frames || !thr || !dec) return "null argument";
    if (recs <= 0 || recs > 65535) return "need 1 <= recs <= 65535";
    if (context < 0 || context > VF_MAX_CONTEXT) return "context must lie in 0 .. 64";
    return nullptr;
}

inline void vf_frame_energy_host(const uint8_t* staged, long long staged_bytes, const int32_t* off, const int32_t* samples, const int32_t* out_off,
                                 int rows, int N, int shift, int channels, int channel, int remove_dc, int max_frames, int64_t* num, double* e) {
    for (int r = 0; r < rows; ++r) {
        const int n = vf_row_samples(off[r], samples[r], channels, staged_bytes);
        const int T = vf_num_frames(n, N, shift, max_frames);
        const uint8_t* x = staged + off[r];
        for (int t = 0; t < T; ++t) {
            long long S1 = 0, S2 = 0;
            for (int i = 0; i < N; ++i) {
                int16_t v;
                memcpy(&v, x + 2 * (((long long)t * shift + i) * channels + channel), 2);
                S1 += v;
                S2 += (long long)v * v;
            }
            const long long m = vf_num(S1, S2, N, remove_dc);
            num[(long long)out_off[r] + t] = m;
            e[(long long)out_off[r] + t] = vf_log_energy(m, N, remove_dc);
        }
    }
}

// thr holds recs thresholds (the device entry keeps its partial sums behind them; the twin adds from the first frame to the last)
inline void vf_decide_host(const double* e, const int32_t* rec_off, const int32_t* rec_frames, int recs, double thr0, double mean_scale,
                           int context, double proportion, double* thr, uint8_t* dec) {
    for (int i = 0; i < recs; ++i) {
        const int T = rec_frames[i] < 0 ? 0 : rec_frames[i];
        const double* x = e + rec_off[i];
        double sum = 0.0;
        for (int t = 0; t < T; ++t) sum += x[t];
        thr[i] = vf_threshold(thr0, mean_scale, sum, T);
        for (int t = 0; t < T; ++t) dec[(long long)rec_off[i] + t] = (uint8_t)vf_vote(x, T, t, context, thr[i], proportion);
    }
}
