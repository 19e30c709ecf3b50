// Kaldi's matrix compression (the inverse of rowops.hip's unpack_compressed_kernel) and the CMVN sums of what an archive holds: the
// arithmetic the kernels (feats.hip) and the serial host twins (cn_compress_feats_host / cn_feats_stats_host; tools/feats_check.cpp
// builds them with a plain C++ compiler under sanitizers) are both made of.  The contract is in include/cassnat_hip_feats.h, the
// definition in DESIGN.md 7n; tests/feats_model.py restates it in numpy.
//
// Every float32 operation is rounded on its own.  On the device that needs saying: hipcc contracts a product and a sum into one FMA,
// so the products go through cn_mul_rn (common.h) and the sums, differences and quotients through __fadd_rn / __fsub_rn / __fdiv_rn;
// x86-64 host code has no fused instruction to contract into.  The reader's own dequantisation (uc_scale / uc_linear / uc_byte, which
// rowops.hip's kernel reads archives with) lives here too, so that P0..P100 are computed by the function that will read them back.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include "common.h"
#define FC_HD __host__ __device__ __forceinline__
#else
#define FC_HD inline
#endif

constexpr int FC_SLAB = 16;       // columns of one workgroup: 64 bytes of every row
constexpr int FC_THREADS = 256;   // 16 columns x 16 rows per step
constexpr int FC_TILE = 64;       // rows of the byte tile that turns row-major values into column-major bytes
constexpr int FC_OK = 0, FC_NO_ROWS = 1, FC_NOT_FINITE = 2, FC_BAD_SPAN = 3;  // the status words

// ---- the reader's dequantisation (formats 1, 2 and 3) --------------------------------------------------------------------------------
FC_HD float uc_scale(float range, float k) {
#pragma clang fp contract(off)
    return range * k;
}
FC_HD float uc_linear(float mn, float inc, unsigned v) {  // uint16 (formats 1 headers, 2) / uint8 (format 3) -> float
#pragma clang fp contract(off)
    return mn + inc * (float)v;
}
FC_HD float uc_byte(float p0, float p25, float p75, float p100, unsigned b) {  // format 1: CharToFloat
#pragma clang fp contract(off)
    if (b <= 64) return p0 + ((p25 - p0) * (float)b) * (1 / 64.0f);
    if (b <= 192) return p25 + ((p75 - p25) * (float)(b - 64)) * (1 / 128.0f);
    return p75 + ((p100 - p75) * (float)(b - 192)) * (1 / 63.0f);
}

// ---- the writer's arithmetic -----------------------------------------------------------------------------------------------------------
FC_HD float fc_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
FC_HD float fc_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
FC_HD float fc_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
FC_HD float fc_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return cn_mul_rn(a, b);
#else
    return a * b;
#endif
}
FC_HD bool fc_finite(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}
// clamp(int(d), 0, hi) with a truncating conversion, defined for every double: a NaN and everything below 1 give 0
FC_HD int fc_trunc_clamp(double d, int hi) {
    if (!(d >= 1.0)) return 0;
    if (d >= (double)hi) return hi;
    return (int)d;
}
FC_HD int64_t fc_bytes(int T, int F) {
    if (T < 0 || F < 1) return 0;
    return T > 8 ? 16 + 8 * (int64_t)F + (int64_t)T * F : 16 + 2 * (int64_t)T * F;
}
FC_HD int fc_clamp_len(int len, int Tmax) { return len > Tmax ? Tmax : len; }
// does utterance r's payload of `bytes` bytes lie inside the output buffer at a multiple of 16?
FC_HD bool fc_span_ok(int64_t off, int64_t bytes, int64_t out_bytes) { return off >= 0 && (off & 15) == 0 && off <= out_bytes - bytes; }

// the global header's two floats from the extremes of the valid rows: a zero minimum is written as +0 (whichever zero came first)
struct FcRange {
    float mn, range;
};
FC_HD FcRange fc_range(float mn, float mx) {
    mn = fc_add(mn, 0.0f);
    if (mx == mn) mx = fc_add(mn, fc_add(1.0f, mn < 0 ? -mn : mn));
    FcRange r;
    r.mn = mn, r.range = fc_sub(mx, mn);
    return r;
}
// float -> uint16 code: monotone non-decreasing in v
FC_HD int fc_u16(float v, float mn, float range) {
    float f = fc_div(fc_sub(v, mn), range);
    f = f < 0.0f ? 0.0f : (f > 1.0f ? 1.0f : f);
    return fc_trunc_clamp((double)fc_mul(f, 65535.0f) + 0.499, 65535);
}
// a column's header from the codes of its sorted values at 0, T / 4, 3 * (T / 4) and T - 1: forced strictly increasing
struct FcColumn {
    int h[4];
    float p[4];  // P0, P25, P75, P100 as the reader dequantises them
};
FC_HD FcColumn fc_column(int c0, int c25, int c75, int c100, float mn, float range) {
    FcColumn k;
    k.h[0] = c0 < 65532 ? c0 : 65532;
    k.h[1] = c25 > k.h[0] + 1 ? c25 : k.h[0] + 1;
    k.h[1] = k.h[1] < 65533 ? k.h[1] : 65533;
    k.h[2] = c75 > k.h[1] + 1 ? c75 : k.h[1] + 1;
    k.h[2] = k.h[2] < 65534 ? k.h[2] : 65534;
    k.h[3] = c100 > k.h[2] + 1 ? c100 : k.h[2] + 1;
    const float inc = uc_scale(range, 1.52590218966964e-05f);
    for (int i = 0; i < 4; ++i) k.p[i] = uc_linear(mn, inc, (unsigned)k.h[i]);
    return k;
}
FC_HD int fc_segment(float v, float lo, float hi, float codes, int top) {
    return fc_trunc_clamp((double)fc_mul(fc_div(fc_sub(v, lo), fc_sub(hi, lo)), codes) + 0.5, top);
}
FC_HD int fc_byte(float v, const float* p) {
    if (v < p[1]) return fc_segment(v, p[0], p[1], 64.0f, 64);
    if (v < p[2]) return 64 + fc_segment(v, p[1], p[2], 128.0f, 128);
    return 192 + fc_segment(v, p[2], p[3], 63.0f, 63);
}

// ---- the serial twins (host only) ------------------------------------------------------------------------------------------------------
#include <algorithm>
#include <vector>

// -> 0; utterance r's payload at out + out_off[r], its status word in status[r].  A payload whose status is not 0 is not written.
static inline int fc_compress_host(const float* feats, const int32_t* lens, const int32_t* out_off, int rows, int Tmax, int F, uint8_t* out,
                                   int64_t out_bytes, int32_t* status) {
    std::vector<uint16_t> codes;
    for (int r = 0; r < rows; ++r) {
        const int T = fc_clamp_len(lens[r], Tmax);
        if (T < 1) {
            status[r] = FC_NO_ROWS;
            continue;
        }
        if (!fc_span_ok(out_off[r], fc_bytes(T, F), out_bytes)) {
            status[r] = FC_BAD_SPAN;
            continue;
        }
        const float* x = feats + (size_t)r * Tmax * F;
        const size_t n = (size_t)T * F;
        float mn = x[0], mx = x[0];
        bool finite = true;
        for (size_t i = 0; i < n; ++i) {
            finite = finite && fc_finite(x[i]);
            mn = x[i] < mn ? x[i] : mn;
            mx = x[i] > mx ? x[i] : mx;
        }
        const FcRange g = fc_range(mn, mx);
        if (!finite || !fc_finite(g.range)) {
            status[r] = FC_NOT_FINITE;
            continue;
        }
        status[r] = FC_OK;
        uint8_t* p = out + out_off[r];
        const int32_t dims[2] = {T, F};
        memcpy(p, &g.mn, 4), memcpy(p + 4, &g.range, 4), memcpy(p + 8, dims, 8);
        if (T <= 8) {
            for (size_t i = 0; i < n; ++i) {
                const uint16_t u = (uint16_t)fc_u16(x[i], g.mn, g.range);
                memcpy(p + 16 + 2 * i, &u, 2);
            }
            continue;
        }
        codes.resize(T);
        const int q = T / 4;
        uint8_t* data = p + 16 + 8 * (size_t)F;
        for (int c = 0; c < F; ++c) {
            for (int t = 0; t < T; ++t) codes[t] = (uint16_t)fc_u16(x[(size_t)t * F + c], g.mn, g.range);
            std::sort(codes.begin(), codes.end());
            const FcColumn k = fc_column(codes[0], codes[q], codes[3 * q], codes[T - 1], g.mn, g.range);
            for (int i = 0; i < 4; ++i) {
                const uint16_t u = (uint16_t)k.h[i];
                memcpy(p + 16 + 8 * (size_t)c + 2 * i, &u, 2);
            }
            for (int t = 0; t < T; ++t) data[(size_t)c * T + t] = (uint8_t)fc_byte(x[(size_t)t * F + c], k.p);
        }
    }
    return 0;
}

// a column's sums in the kernel's order: sixteen partial sums, row t into partial t % 16, then the partials added from the first to
// the last - so that the twin gives the kernel's bits (a square of a float32 value is exact in float64, fused or not)
struct FcSums {
    double s[16], ss[16];
    FcSums() {
        for (int k = 0; k < 16; ++k) s[k] = ss[k] = 0.0;
    }
    void add(int t, double v) { s[t & 15] += v, ss[t & 15] += v * v; }
    void total(double* sum, double* sumsq) const {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < 16; ++k) a += s[k], b += ss[k];
        *sum = a, *sumsq = b;
    }
};

// stats[r][0][c] / stats[r][1][c]: the float64 sum and sum of squares of column c of what the archive holds of utterance r - with
// `payload` the values a reader dequantises from the payload at out_off[r], without it the float32 rows.  An utterance without rows,
// or whose status (when given) is not 0, gives zeros.
static inline int fc_stats_host(const float* feats, const uint8_t* payload, const int32_t* out_off, const int32_t* lens, const int32_t* status,
                                int rows, int Tmax, int F, double* stats) {
    for (int r = 0; r < rows; ++r) {
        double* s = stats + (size_t)r * 2 * F;
        for (int i = 0; i < 2 * F; ++i) s[i] = 0.0;
        const int T = fc_clamp_len(lens[r], Tmax);
        if (T < 1 || (status && status[r] != FC_OK)) continue;
        if (!payload) {
            const float* x = feats + (size_t)r * Tmax * F;
            for (int c = 0; c < F; ++c) {
                FcSums k;
                for (int t = 0; t < T; ++t) k.add(t, x[(size_t)t * F + c]);
                k.total(&s[c], &s[F + c]);
            }
            continue;
        }
        const uint8_t* p = payload + out_off[r];
        float mn, range;
        memcpy(&mn, p, 4), memcpy(&range, p + 4, 4);
        const float inc = uc_scale(range, 1.52590218966964e-05f);
        for (int c = 0; c < F; ++c) {
            uint16_t h[4] = {0, 0, 0, 0};
            float q[4] = {0, 0, 0, 0};
            if (T > 8) {
                memcpy(h, p + 16 + 8 * (size_t)c, 8);
                for (int i = 0; i < 4; ++i) q[i] = uc_linear(mn, inc, h[i]);
            }
            FcSums k;
            for (int t = 0; t < T; ++t) {
                double v;
                if (T > 8) {
                    v = uc_byte(q[0], q[1], q[2], q[3], p[16 + 8 * (size_t)F + (size_t)c * T + t]);
                } else {
                    uint16_t u;
                    memcpy(&u, p + 16 + 2 * ((size_t)t * F + c), 2);
                    v = uc_linear(mn, inc, u);
                }
                k.add(t, v);
            }
            k.total(&s[c], &s[F + c]);
        }
    }
    return 0;
}
