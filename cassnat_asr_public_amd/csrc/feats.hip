// Feature archives written on the device (bin/make_fbank): Kaldi's matrix compression behind the fbank kernel - the inverse of
// rowops.hip's unpack_compressed_kernel - and the CMVN sums of what the archive then holds.  feats_compress.h holds the arithmetic
// (the same functions the serial host twins run), include/cassnat_hip_feats.h the contract, DESIGN.md 7n the definition.
//
// The batch arrives row-major (rows, Tmax, F) and format 1 wants column statistics and column-major bytes.  A workgroup owns one
// utterance and a slab of 16 columns - 64 bytes of every row: thread (c = tid & 15, tl = tid >> 4) reads column c of rows tl, tl + 16,
// ..., so sixteen lanes read one contiguous 64-byte segment and a wave four rows' segments; no lane walks a column at a row's stride.
//   feats_range_kernel   one workgroup of 1024 threads per utterance over its T * F contiguous values, 16 bytes per lane and load:
//                        minimum, maximum, a non-finite flag; lane 0
//                        writes the status word and, for a good utterance, the 16-byte global header.
//   feats_encode_kernel  (utterance, slab).  T <= 8: the uint16 codes, row-major (format 2).  Else the four order statistics are
//                        selected over the 16-bit CODES, which are monotone in the value: minimum and maximum of the codes by LDS
//                        integer atomics, the ranks T / 4 and 3 * (T / 4) by two 8-bit histogram passes per column in LDS - the high
//                        bytes, then the low bytes of the codes that share the selected high byte - with no sort.  The bytes go
//                        through a 16 x 64 LDS tile and leave column-major, sixteen lanes writing sixteen consecutive bytes.
//   feats_stats_kernel   (utterance, slab): float64 sums and sums of squares, sixteen partial sums per column added in a fixed order -
//                        no atomics, the same bits in every run.
// All LDS atomics are integer adds / min / max: their result does not depend on the order.  Every read stays in the valid rows of
// the utterance, every write inside the payload whose span the range kernel has checked against the output buffer.
#include "feats_compress.h"

#include "../../include/cassnat_hip_feats.h"

constexpr int FC_RANGE_THREADS = 1024;  // one workgroup per utterance: sixteen waves, 16 bytes per lane and load

struct FcExtremes {
    float mn, mx;
    int bad;
    __device__ __forceinline__ void take(float v) {
        bad |= !fc_finite(v);
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
};

__global__ __launch_bounds__(FC_RANGE_THREADS) void feats_range_kernel(const float* __restrict__ feats, const int* __restrict__ lens,
                                                                       const int* __restrict__ out_off, int Tmax, int F,
                                                                       unsigned char* __restrict__ out, long long out_bytes, int* __restrict__ status) {
    __shared__ float smn[FC_RANGE_THREADS / 64], smx[FC_RANGE_THREADS / 64];
    __shared__ int sbad[FC_RANGE_THREADS / 64];
    const int r = blockIdx.x;
    const int T = fc_clamp_len(lens[r], Tmax);
    const long long off = out_off[r];
    if (T < 1 || !fc_span_ok(off, fc_bytes(T, F), out_bytes)) {  // (uniform over the workgroup)
        if (threadIdx.x == 0) status[r] = T < 1 ? FC_NO_ROWS : FC_BAD_SPAN;
        return;
    }
    const float* x = feats + (long long)r * Tmax * F;
    const long long n = (long long)T * F;
    // the valid rows are contiguous: scalars up to the first 16-byte boundary, 16 bytes per lane from there (four loads in flight), the rest
    long long head = (4 - (long long)(((size_t)x >> 2) & 3)) & 3;
    head = head < n ? head : n;
    const long long quads = (n - head) >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x + head);
    FcExtremes e = {__builtin_inff(), -__builtin_inff(), 0};
    if (threadIdx.x < head) e.take(x[threadIdx.x]);
#pragma unroll 4
    for (long long i = threadIdx.x; i < quads; i += FC_RANGE_THREADS) {
        const f32x4 v = x4[i];
        e.take(v[0]), e.take(v[1]), e.take(v[2]), e.take(v[3]);
    }
    const long long tail = head + 4 * quads + threadIdx.x;
    if (tail < n) e.take(x[tail]);
    float mn = e.mn, mx = e.mx;
    int bad = e.bad;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
        bad |= __shfl_xor(bad, d);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6] = mn, smx[threadIdx.x >> 6] = mx, sbad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < FC_RANGE_THREADS / 64; ++w) {
        mn = smn[w] < mn ? smn[w] : mn;
        mx = smx[w] > mx ? smx[w] : mx;
        bad |= sbad[w];
    }
    const FcRange g = fc_range(mn, mx);
    if (bad || !fc_finite(g.range)) {
        status[r] = FC_NOT_FINITE;
        return;
    }
    status[r] = FC_OK;
    const uint4 head16 = {__float_as_uint(g.mn), __float_as_uint(g.range), (unsigned)T, (unsigned)F};
    *reinterpret_cast<uint4*>(out + off) = head16;
}

// the bin of a 256-bin histogram (one column's: stride FC_SLAB) that holds rank k, and the rank inside it
__device__ __forceinline__ void fc_select(const unsigned* hist, int k, int* bin, int* rest) {
    int cum = 0, b = 0;
    for (; b < 255; ++b) {
        const int n = (int)hist[b * FC_SLAB];
        if (cum + n > k) break;
        cum += n;
    }
    *bin = b, *rest = k - cum;
}

// rows t0, t0 + 16, t0 + 32, t0 + 48 of a thread's column, the loads issued together (rows at or behind T are not read)
constexpr int FC_ROWS_PER_STEP = 4 * (FC_THREADS / FC_SLAB);
__device__ __forceinline__ void fc_load4(float (&v)[4], const float* x, int t0, int T, int F) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = t0 + 16 * k < T ? x[(long long)(t0 + 16 * k) * F] : 0.f;
}

__global__ __launch_bounds__(FC_THREADS) void feats_encode_kernel(const float* __restrict__ feats, const int* __restrict__ lens,
                                                                  const int* __restrict__ out_off, int Tmax, int F,
                                                                  unsigned char* __restrict__ out, const int* __restrict__ status) {
    __shared__ unsigned hist_hi[256 * FC_SLAB];
    __shared__ unsigned hist_lo[2][256 * FC_SLAB];
    __shared__ int cmin[FC_SLAB], cmax[FC_SLAB], sel[2][FC_SLAB], rest[2][FC_SLAB], quart[2][FC_SLAB];
    __shared__ float P[FC_SLAB][4];
    __shared__ unsigned char tile[FC_SLAB][FC_TILE];
    const int r = blockIdx.x, c0 = blockIdx.y * FC_SLAB, tid = threadIdx.x;
    if (status[r] != FC_OK) return;  // (uniform; the range kernel has checked the rows and the span)
    const int T = fc_clamp_len(lens[r], Tmax);
    const int cn = (F - c0) < FC_SLAB ? (F - c0) : FC_SLAB;
    const int c = tid & (FC_SLAB - 1), tl = tid >> 4;
    const bool active = c < cn;
    const float* x = feats + (long long)r * Tmax * F + c0 + c;
    unsigned char* p = out + (long long)out_off[r];
    const float mn = *reinterpret_cast<const float*>(p), range = *reinterpret_cast<const float*>(p + 4);  // (the range kernel's)
    if (T <= 8) {  // format 2: uint16, row-major
        unsigned short* d = reinterpret_cast<unsigned short*>(p + 16) + c0 + c;
        if (active && tl < T) d[(long long)tl * F] = (unsigned short)fc_u16(x[(long long)tl * F], mn, range);
        return;
    }
    for (int i = tid; i < 256 * FC_SLAB; i += FC_THREADS) hist_hi[i] = 0, hist_lo[0][i] = 0, hist_lo[1][i] = 0;
    if (tid < FC_SLAB) cmin[tid] = 65535, cmax[tid] = 0;
    __syncthreads();
    // pass 1: the high bytes, and the extremes of the codes
    if (active) {
        int lo = 65535, hi = 0;
        for (int t0 = tl; t0 < T; t0 += FC_ROWS_PER_STEP) {  // (four rows' loads in flight)
            float v[4];
            fc_load4(v, x, t0, T, F);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t0 + 16 * k >= T) break;
                const int code = fc_u16(v[k], mn, range);
                atomicAdd(&hist_hi[(code >> 8) * FC_SLAB + c], 1u);
                lo = code < lo ? code : lo;
                hi = code > hi ? code : hi;
            }
        }
        atomicMin(&cmin[c], lo);
        atomicMax(&cmax[c], hi);
    }
    __syncthreads();
    const int q = T / 4;
    if (tid < 2 * FC_SLAB) fc_select(hist_hi + (tid & (FC_SLAB - 1)), (tid >> 4) ? 3 * q : q, &sel[tid >> 4][tid & (FC_SLAB - 1)], &rest[tid >> 4][tid & (FC_SLAB - 1)]);
    __syncthreads();
    // pass 2: the low bytes of the codes under the two selected high bytes
    if (active) {
        const int s0 = sel[0][c], s1 = sel[1][c];
        for (int t0 = tl; t0 < T; t0 += FC_ROWS_PER_STEP) {
            float v[4];
            fc_load4(v, x, t0, T, F);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t0 + 16 * k >= T) break;
                const int code = fc_u16(v[k], mn, range);
                if ((code >> 8) == s0) atomicAdd(&hist_lo[0][(code & 255) * FC_SLAB + c], 1u);
                if ((code >> 8) == s1) atomicAdd(&hist_lo[1][(code & 255) * FC_SLAB + c], 1u);
            }
        }
    }
    __syncthreads();
    if (tid < 2 * FC_SLAB) {
        int bin, left;
        fc_select(hist_lo[tid >> 4] + (tid & (FC_SLAB - 1)), rest[tid >> 4][tid & (FC_SLAB - 1)], &bin, &left);
        quart[tid >> 4][tid & (FC_SLAB - 1)] = (sel[tid >> 4][tid & (FC_SLAB - 1)] << 8) | bin;
    }
    __syncthreads();
    if (tid < cn) {
        const FcColumn k = fc_column(cmin[tid], quart[0][tid], quart[1][tid], cmax[tid], mn, range);
        const uint2 h = {(unsigned)k.h[0] | ((unsigned)k.h[1] << 16), (unsigned)k.h[2] | ((unsigned)k.h[3] << 16)};
        *reinterpret_cast<uint2*>(p + 16 + 8 * (long long)(c0 + tid)) = h;
#pragma unroll
        for (int i = 0; i < 4; ++i) P[tid][i] = k.p[i];
    }
    __syncthreads();
    // pass 3: the bytes, 64 rows at a time through the tile
    unsigned char* data = p + 16 + 8 * (long long)F;
    const int wc = tid >> 4, wj = tid & 15;  // the writer's column and place in a run of 16 bytes
    const float pc[4] = {P[c][0], P[c][1], P[c][2], P[c][3]};
    for (int t0 = 0; t0 < T; t0 += FC_TILE) {
#pragma unroll
        for (int k = 0; k < FC_TILE / 16; ++k) {
            const int t = t0 + tl + 16 * k;
            if (active && t < T) tile[c][tl + 16 * k] = (unsigned char)fc_byte(x[(long long)t * F], pc);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FC_TILE / 16; ++k) {
            const int t = t0 + 16 * k + wj;
            if (wc < cn && t < T) data[(long long)(c0 + wc) * T + t] = tile[wc][16 * k + wj];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(FC_THREADS) void feats_stats_kernel(const float* __restrict__ feats, const unsigned char* __restrict__ payload,
                                                                 const int* __restrict__ out_off, const int* __restrict__ lens,
                                                                 const int* __restrict__ status, int Tmax, int F, double* __restrict__ stats) {
    __shared__ double part[2][FC_SLAB][FC_THREADS / FC_SLAB + 1];
    const int r = blockIdx.x, c0 = blockIdx.y * FC_SLAB, tid = threadIdx.x;
    const int T = fc_clamp_len(lens[r], Tmax);
    const int cn = (F - c0) < FC_SLAB ? (F - c0) : FC_SLAB;
    double* dst = stats + (long long)r * 2 * F + c0;
    if (T < 1 || (status && status[r] != FC_OK)) {  // (uniform)
        if (tid < cn) dst[tid] = 0.0, dst[F + tid] = 0.0;
        return;
    }
    double s = 0.0, ss = 0.0;
    int col, slot;
    if (payload && T > 8) {  // format 1: a column's bytes are contiguous - sixteen lanes along time
        col = tid >> 4, slot = tid & 15;
        if (col < cn) {
            const unsigned char* p = payload + (long long)out_off[r];
            const float mn = *reinterpret_cast<const float*>(p), inc = uc_scale(*reinterpret_cast<const float*>(p + 4), 1.52590218966964e-05f);
            const unsigned short* h = reinterpret_cast<const unsigned short*>(p + 16) + 4 * (long long)(c0 + col);
            const float p0 = uc_linear(mn, inc, h[0]), p25 = uc_linear(mn, inc, h[1]), p75 = uc_linear(mn, inc, h[2]), p100 = uc_linear(mn, inc, h[3]);
            const unsigned char* d = p + 16 + 8 * (long long)F + (long long)(c0 + col) * T;
            for (int t = slot; t < T; t += 16) {
                const double v = (double)uc_byte(p0, p25, p75, p100, d[t]);
                s += v, ss += v * v;
            }
        }
    } else {  // row-major: format 2's uint16, or the float32 rows
        col = tid & 15, slot = tid >> 4;
        if (col < cn) {
            if (payload) {
                const unsigned char* p = payload + (long long)out_off[r];
                const float mn = *reinterpret_cast<const float*>(p), inc = uc_scale(*reinterpret_cast<const float*>(p + 4), 1.52590218966964e-05f);
                const unsigned short* d = reinterpret_cast<const unsigned short*>(p + 16) + c0 + col;
                for (int t = slot; t < T; t += 16) {
                    const double v = (double)uc_linear(mn, inc, d[(long long)t * F]);
                    s += v, ss += v * v;
                }
            } else {
                const float* x = feats + (long long)r * Tmax * F + c0 + col;
                for (int t = slot; t < T; t += 16) {
                    const double v = (double)x[(long long)t * F];
                    s += v, ss += v * v;
                }
            }
        }
    }
    part[0][col][slot] = s, part[1][col][slot] = ss;
    __syncthreads();
    if (tid < cn) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < FC_THREADS / FC_SLAB; ++k) a += part[0][tid][k], b += part[1][tid][k];
        dst[tid] = a, dst[F + tid] = b;
    }
}

static int fc_check(const char* who, const void* a, const void* b, const void* c, int rows, int Tmax, int F) {
    if (!a || !b || !c) {
        cn_set_error(std::string(who) + ": null argument");
        return -1;
    }
    if (rows < 1 || Tmax < 1 || F < 1 || F > FC_SLAB * 65535) {
        cn_set_error(std::string(who) + ": need rows, Tmax >= 1 and 1 <= F <= " + std::to_string(FC_SLAB * 65535));
        return -1;
    }
    return 0;
}

extern "C" int64_t cn_compress_feats_bytes(int32_t T, int32_t F) { return fc_bytes(T, F); }

extern "C" int cn_op_compress_feats(const float* feats_dev, const int32_t* lens_dev, const int32_t* out_off_dev, int32_t rows, int32_t Tmax,
                                    int32_t F, void* out_dev, int64_t out_bytes, int32_t* status_dev, void* stream) {
    CN_TRY(fc_check("cn_op_compress_feats", feats_dev, lens_dev, out_off_dev, rows, Tmax, F));
    if (!out_dev || !status_dev || out_bytes < 0 || ((size_t)out_dev & 15) || ((size_t)feats_dev & 3)) {
        cn_set_error("cn_op_compress_feats: the output buffer must exist and start on a 16-byte boundary, the batch on a 4-byte one");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned char* out = static_cast<unsigned char*>(out_dev);
    hipLaunchKernelGGL(feats_range_kernel, dim3((unsigned)rows), dim3(FC_RANGE_THREADS), 0, s, feats_dev, lens_dev, out_off_dev, Tmax, F, out,
                       (long long)out_bytes, status_dev);
    CN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(feats_encode_kernel, dim3((unsigned)rows, (unsigned)cn_ceil_div(F, FC_SLAB)), dim3(FC_THREADS), 0, s, feats_dev, lens_dev,
                       out_off_dev, Tmax, F, out, status_dev);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cn_compress_feats_host(const float* feats, const int32_t* lens, const int32_t* out_off, int32_t rows, int32_t Tmax, int32_t F,
                                      void* out, int64_t out_bytes, int32_t* status) {
    CN_TRY(fc_check("cn_compress_feats_host", feats, lens, out_off, rows, Tmax, F));
    if (!out || !status || out_bytes < 0) {
        cn_set_error("cn_compress_feats_host: null argument");
        return -1;
    }
    return fc_compress_host(feats, lens, out_off, rows, Tmax, F, static_cast<uint8_t*>(out), out_bytes, status);
}

extern "C" int cn_op_feats_stats(const float* feats_dev, const void* payload_dev, const int32_t* out_off_dev, const int32_t* lens_dev,
                                 const int32_t* status_dev, int32_t rows, int32_t Tmax, int32_t F, double* stats_dev, void* stream) {
    CN_TRY(fc_check("cn_op_feats_stats", payload_dev ? payload_dev : feats_dev, lens_dev, stats_dev, rows, Tmax, F));
    if (payload_dev && (!out_off_dev || ((size_t)payload_dev & 15))) {
        cn_set_error("cn_op_feats_stats: payloads need their offsets and a buffer that starts on a 16-byte boundary");
        return -1;
    }
    hipLaunchKernelGGL(feats_stats_kernel, dim3((unsigned)rows, (unsigned)cn_ceil_div(F, FC_SLAB)), dim3(FC_THREADS), 0, (hipStream_t)stream,
                       feats_dev, static_cast<const unsigned char*>(payload_dev), out_off_dev, lens_dev, status_dev, Tmax, F, stats_dev);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int cn_feats_stats_host(const float* feats, const void* payload, const int32_t* out_off, const int32_t* lens, const int32_t* status,
                                   int32_t rows, int32_t Tmax, int32_t F, double* stats) {
    CN_TRY(fc_check("cn_feats_stats_host", payload ? payload : feats, lens, stats, rows, Tmax, F));
    if (payload && !out_off) {
        cn_set_error("cn_feats_stats_host: payloads need their offsets");
        return -1;
    }
    return fc_stats_host(feats, static_cast<const uint8_t*>(payload), out_off, lens, status, rows, Tmax, F, stats);
}
