// C-ABI entry points of libcassnat_hip.so that take no model handle: the Kaldi fbank front end and the resampler in front of it, the host gather of the packed
// reader and the single-kernel entries (cn_op_*) through which the tests drive every hand-written kernel.  See
// include/cassnat_hip.h for the contract; the handle is handle.hip, weight packing weights.hip, the decode paths
// model.hip / decode_ar.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cassnat_hip.h"
#include "../../include/cassnat_hip_align.h"
#include "../../include/cassnat_hip_attention_proj.h"
#include "../../include/cassnat_hip_genmax.h"
#include "ctc_search_host.h"
#include "ctc_times_search.h"
#include "edit_align_search.h"
#include "flac_decode.h"
#include "kernels.h"

namespace {

// Device scratch of one entry: alloc / upload, launch, then finish(rc).  The destructor drains the stream and frees every
// buffer, so each exit path - a failed hip call after the first allocation included - gives them back.
class Scratch {
  public:
    Scratch(const char* who, hipStream_t s) : who_(who), s_(s) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        (void)hipStreamSynchronize(s_);
        for (void* p : bufs_) (void)hipFree(p);
    }
    // false (error set) once an allocation or upload of this guard failed; the later ones are not attempted
    bool ok() const { return ok_; }
    void* alloc(size_t bytes) {
        if (!ok_) return nullptr;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail("hipMalloc", bytes, e);
        bufs_.push_back(p);
        return p;
    }
    void* upload(const void* host, size_t bytes) {
        void* p = alloc(bytes);
        if (!p) return nullptr;
        const hipError_t e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? p : fail("hipMemcpy", bytes, e);
    }
    // rc of the launches, or -2 (error set) when they were accepted and the stream then failed
    int finish(int rc) {
        const hipError_t e = hipStreamSynchronize(s_);
        if (rc == 0 && e != hipSuccess) {
            cn_set_error(std::string(who_) + ": " + hipGetErrorString(e));
            return -2;
        }
        return rc;
    }

  private:
    void* fail(const char* what, size_t bytes, hipError_t e) {
        cn_set_error(std::string(who_) + ": " + what + " of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
        ok_ = false;
        return nullptr;
    }
    const char* who_;
    hipStream_t s_;
    std::vector<void*> bufs_;
    bool ok_ = true;
};

// fp32 [M][256] -> split-bf16 rows (hi + lo halves, 1 KiB per row) as the split-bf16 kernels read them
std::vector<unsigned char> split_rows256(const float* x, int M) {
    std::vector<unsigned char> hx((size_t)M * 1024);
    for (size_t r = 0; r < (size_t)M; ++r)
        for (size_t c = 0; c < 256; ++c) {
            const float v = x[r * 256 + c];
            const uint16_t hi = cn_host_op16(v);
            const uint32_t hbits = (uint32_t)hi << 16;
            float hf;
            std::memcpy(&hf, &hbits, 4);
            const uint16_t lo = cn_host_op16(v - hf);
            std::memcpy(&hx[r * 1024 + cn_split_off(c)], &hi, 2);
            std::memcpy(&hx[r * 1024 + cn_split_off(c) + 64], &lo, 2);
        }
    return hx;
}

}  // namespace

// ---- single-kernel entry points ------------------------------------------------------------------
static FbankOpts fbank_opts_from(const cn_fbank_opts* o) {
    FbankOpts f;
    f.sample_rate = o->sample_rate;
    f.frame_length_ms = o->frame_length_ms;
    f.frame_shift_ms = o->frame_shift_ms;
    f.preemph = o->preemph;
    f.low_freq = o->low_freq;
    f.high_freq = o->high_freq;
    f.num_mel = o->num_mel;
    f.window_type = o->window_type;
    f.remove_dc = o->remove_dc;
    f.use_power = o->use_power;
    f.use_log = o->use_log;
    return f;
}

extern "C" void cn_fbank_default_opts(cn_fbank_opts* o) {
    if (!o) return;
    const FbankOpts f;
    std::memset(o, 0, sizeof(*o));
    o->sample_rate = f.sample_rate;
    o->frame_length_ms = f.frame_length_ms;
    o->frame_shift_ms = f.frame_shift_ms;
    o->preemph = f.preemph;
    o->low_freq = f.low_freq;
    o->high_freq = f.high_freq;
    o->num_mel = f.num_mel;
    o->window_type = f.window_type;
    o->remove_dc = f.remove_dc;
    o->use_power = f.use_power;
    o->use_log = f.use_log;
}

extern "C" int32_t cn_fbank_num_frames(const cn_fbank_opts* o, int32_t num_samples) {
    return o ? fbank_num_frames(fbank_opts_from(o), num_samples) : 0;
}

extern "C" int cn_fbank(const cn_fbank_opts* o, const float* wave_dev, const int32_t* num_samples_dev, int32_t B,
                        int32_t max_samples, const float* cmvn_mean_dev, const float* cmvn_istd_dev, float* feats_dev,
                        int32_t Tmax, float pad_value, void* stream) {
    if (!o || !wave_dev || !num_samples_dev || !feats_dev || B < 0 || max_samples < 0 || Tmax < 0) {
        cn_set_error("cn_fbank: bad argument");
        return -1;
    }
    return launch_fbank(fbank_opts_from(o), wave_dev, num_samples_dev, B, max_samples, cmvn_mean_dev, cmvn_istd_dev, feats_dev,
                        Tmax, pad_value, (hipStream_t)stream);
}

static int fbank_packed_entry(const char* who, const cn_fbank_opts* o, const void* staged_dev, int64_t staged_bytes, const int32_t* off_dev,
                              const int32_t* samples_dev, float* out_dev, int32_t rows, int32_t T, float pad, const double* mean_dev,
                              const double* std_dev, bool f32, void* stream) {
    if (!o || !staged_dev || !off_dev || !samples_dev || !out_dev || (!mean_dev) != (!std_dev)) {
        cn_set_error(std::string(who) + ": null argument (mean and std come together)");
        return -1;
    }
    if (rows <= 0 || T <= 0 || o->num_mel <= 0 || staged_bytes < 0) {
        cn_set_error(std::string(who) + ": rows, T and num_mel must be positive");
        return -1;
    }
    const FbankOpts f = fbank_opts_from(o);
    if (fbank_frame_samples(f) > 512) {
        cn_set_error(std::string(who) + ": a frame of more than 512 samples does not fit the 512-point FFT");
        return -1;
    }
    return launch_fbank_packed(f, static_cast<const unsigned char*>(staged_dev), staged_bytes, off_dev, samples_dev, out_dev, rows, T, pad,
                               mean_dev, std_dev, f32, (hipStream_t)stream);
}

extern "C" int cn_op_fbank_packed(const cn_fbank_opts* o, const void* staged_dev, int64_t staged_bytes, const int32_t* off_dev,
                                  const int32_t* samples_dev, float* out_dev, int32_t rows, int32_t T, float pad, const double* mean_dev,
                                  const double* std_dev, void* stream) {
    return fbank_packed_entry("cn_op_fbank_packed", o, staged_dev, staged_bytes, off_dev, samples_dev, out_dev, rows, T, pad, mean_dev, std_dev,
                              false, stream);
}

extern "C" int cn_op_fbank_packed_f32(const cn_fbank_opts* o, const void* wave_dev, int64_t wave_bytes, const int32_t* off_dev,
                                      const int32_t* samples_dev, float* out_dev, int32_t rows, int32_t T, float pad, const double* mean_dev,
                                      const double* std_dev, void* stream) {
    return fbank_packed_entry("cn_op_fbank_packed_f32", o, wave_dev, wave_bytes, off_dev, samples_dev, out_dev, rows, T, pad, mean_dev, std_dev,
                              true, stream);
}

extern "C" int64_t cn_resample_num_samples(int32_t in_rate, int32_t out_rate, int64_t in_samples) {
    return resample_num_samples(in_rate, out_rate, in_samples);
}

extern "C" int cn_resample_table(int32_t in_rate, int32_t out_rate, int32_t* in_unit, int32_t* out_unit, int32_t* max_taps,
                                 int32_t* first_host, int32_t* taps_host, float* weights_host, int64_t capacity) {
    if (!in_unit || !out_unit || !max_taps) {
        cn_set_error("cn_resample_table: null argument");
        return -1;
    }
    return resample_table(in_rate, out_rate, in_unit, out_unit, max_taps, first_host, taps_host, weights_host, capacity);
}

extern "C" int cn_op_wave_resample(int32_t in_rate, int32_t out_rate, const void* staged_dev, int64_t staged_bytes, const int32_t* off_dev,
                                   const int32_t* samples_dev, const int32_t* channels_dev, const int32_t* channel_dev,
                                   const int32_t* channels_host, const int32_t* channel_host, int32_t utts, const int32_t* rows_dev,
                                   int32_t rows, int64_t max_out, float* wave_dev, const int32_t* out_off_dev, void* stream) {
    if (!staged_dev || !off_dev || !samples_dev || !channels_dev || !channel_dev || !channels_host || !channel_host || !wave_dev ||
        !out_off_dev) {
        cn_set_error("cn_op_wave_resample: null argument");
        return -1;
    }
    if (in_rate <= 0 || out_rate <= 0) {
        cn_set_error("cn_op_wave_resample: the rates must be positive");
        return -1;
    }
    if (utts <= 0 || rows <= 0 || (!rows_dev && rows > utts) || max_out <= 0 || staged_bytes < 0) {
        cn_set_error("cn_op_wave_resample: utts, rows (<= utts without a row list) and max_out must be positive");
        return -1;
    }
    for (int32_t r = 0; r < utts; ++r)
        if (channels_host[r] < 1 || channel_host[r] < 0 || channel_host[r] >= channels_host[r]) {
            cn_set_error("cn_op_wave_resample: utterance #" + std::to_string(r) + ": channel " + std::to_string(channel_host[r]) + " of " +
                         std::to_string(channels_host[r]));
            return -1;
        }
    return launch_wave_resample(in_rate, out_rate, static_cast<const unsigned char*>(staged_dev), staged_bytes, off_dev, samples_dev, channels_dev,
                                channel_dev, utts, rows_dev, rows, max_out, wave_dev, out_off_dev, (hipStream_t)stream);
}

// cn_gemm_desc -> (internal precision, GemmArgs): the checks of the descriptor itself (cassnat_hip.h lists them); the shape and
// stride checks are decide_gemm's, which launch_gemm runs for the engine's calls too.  0, or -1 with the error set.
static int gemm_args_of(const char* who, const cn_gemm_desc* d, int* prec, GemmArgs* g) {
    auto refuse = [&](const char* what) {
        cn_set_error(std::string(who) + ": " + what);
        return -1;
    };
    if (!d) return refuse("null descriptor");
    if (!d->A || !d->W || !d->C) return refuse("null A, W or C");
    if (d->precision != CN_PRECISION_F32 && d->precision != CN_PRECISION_BF16 && d->precision != CN_PRECISION_BF16X3 &&
        d->precision != CN_PRECISION_F16)
        return refuse("precision must be CN_PRECISION_F32, CN_PRECISION_BF16, CN_PRECISION_BF16X3 or CN_PRECISION_F16");
    if ((*prec = cn_own_precision(d->precision, who)) < 0) return -1;
    if (d->reserved != 0) return refuse("the reserved word must be 0");
    if (d->epi & ~(CN_GEMM_EPI_RELU | CN_GEMM_EPI_RESID | CN_GEMM_EPI_EMBED | CN_GEMM_EPI_SWISH)) return refuse("unknown epilogue bits");
    if (d->c_kind != CN_GEMM_OUT_OWN && d->c_kind != CN_GEMM_OUT_F32 && d->c_kind != CN_GEMM_OUT_E4M3)
        return refuse("c_kind must be CN_GEMM_OUT_OWN, CN_GEMM_OUT_F32 or CN_GEMM_OUT_E4M3");
    if (d->c_kind == CN_GEMM_OUT_E4M3 && !d->ab_fp8) return refuse("an e4m3 output needs e4m3 operands (ab_fp8)");
    if (d->ab_fp8 && d->precision != CN_PRECISION_BF16)
        return refuse("e4m3 operands belong to CN_PRECISION_BF16 (the type of their 16-bit output)");
    if (d->M < 0 || d->N < 0) return refuse("M and N must not be negative");
    g->A = d->A;
    g->lda = d->lda;
    g->W = d->W;
    g->bias = d->bias;
    g->C = d->C;
    g->ldc = d->ldc;
    g->c_f32 = d->c_kind == CN_GEMM_OUT_F32;
    g->c_fp8 = d->c_kind == CN_GEMM_OUT_E4M3;
    g->M = d->M;
    g->N = d->N;
    g->K = d->K;
    g->epi = d->epi;
    g->resid = d->resid;
    g->ldr = d->ldr;
    g->resid_scale = d->resid_scale;
    g->pe = d->pe;
    g->pe_period = d->pe_period;
    g->scale = d->scale;
    g->ab_fp8 = d->ab_fp8 != 0;
    g->acc_scale = d->acc_scale;
    g->w_inv_scale = d->w_inv_scale;
    g->c_scale = d->c_scale;
    return 0;
}

static int op_gemm_desc(const char* who, const cn_gemm_desc* d, void* stream) {
    int prec;
    GemmArgs g;
    GemmForm f;
    if (gemm_args_of(who, d, &prec, &g) != 0 || decide_gemm(prec, g, &f, who) != 0) return -1;
    return launch_gemm(prec, g, (hipStream_t)stream);
}

extern "C" int cn_op_gemm_desc(const cn_gemm_desc* d, void* stream) { return op_gemm_desc("cn_op_gemm_desc", d, stream); }
extern "C" int32_t cn_gemm_desc_size(void) { return (int32_t)sizeof(cn_gemm_desc); }
extern "C" int32_t cn_gemm_form(const cn_gemm_desc* d) {
    int prec;
    GemmArgs g;
    GemmForm f;
    if (gemm_args_of("cn_gemm_form", d, &prec, &g) != 0 || decide_gemm(prec, g, &f, "cn_gemm_form") != 0) return -1;
    return f.elem | f.out << 4 | f.tile << 8;
}

static_assert(CN_GEMM_EPI_RELU == CN_EPI_RELU && CN_GEMM_EPI_RESID == CN_EPI_RESID && CN_GEMM_EPI_EMBED == CN_EPI_EMBED &&
                  CN_GEMM_EPI_SWISH == CN_EPI_SWISH,
              "the public epilogue bits are the kernel's");

// cn_op_gemm: the descriptor of a product in the model precision with the epilogues its arguments can name
extern "C" int cn_op_gemm(int32_t precision, const void* A, int32_t lda, const void* W, const float* bias, void* C,
                          int32_t ldc, int32_t c_is_f32, int32_t M, int32_t N, int32_t K, int32_t relu,
                          const float* resid, int32_t ldr, const float* pe, int32_t pe_period, float scale,
                          void* stream) {
    cn_gemm_desc d = {};
    d.precision = precision;
    d.c_kind = c_is_f32 ? CN_GEMM_OUT_F32 : CN_GEMM_OUT_OWN;
    d.A = A;
    d.lda = lda;
    d.W = W;
    d.bias = bias;
    d.C = C;
    d.ldc = ldc;
    d.M = M;
    d.N = N;
    d.K = K;
    d.epi = (relu ? CN_GEMM_EPI_RELU : 0) | (resid ? CN_GEMM_EPI_RESID : 0) | (pe ? CN_GEMM_EPI_EMBED : 0);
    d.resid = resid;
    d.ldr = ldr;
    d.resid_scale = 1.f;
    d.pe = pe;
    d.pe_period = pe_period;
    d.scale = scale;
    d.acc_scale = d.c_scale = 1.f;
    return op_gemm_desc("cn_op_gemm", &d, stream);
}

extern "C" int cn_op_convert(int32_t precision, const void* src, void* dst, int64_t n, int32_t to_f32, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_convert")) < 0) return -1;
    if (n < 0 || !src || !dst) {
        cn_set_error("cn_op_convert: bad argument");
        return -1;
    }
    return to_f32 ? launch_convert_back(precision, src, (float*)dst, (size_t)n, (hipStream_t)stream)
                  : launch_convert(precision, (const float*)src, dst, (size_t)n, (hipStream_t)stream);
}

extern "C" int cn_op_conv1(int32_t precision, const float* x, const float* w9c, const float* bias, void* out, int32_t B,
                           int32_t T, int32_t F, int32_t C, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_conv1")) < 0) return -1;
    return launch_conv1(precision, x, w9c, bias, out, B, T, F, (T - 1) / 2 + 1, (F - 1) / 2 + 1, C, 0, (hipStream_t)stream);
}

// the bf16 engine's bordered image ([B][T1 + 2][F1 + 2][C] bf16, zero border) as conv2's LDS-DMA kernel reads it, from the
// matrix-core kernel (C == 256, (F - 1) / 2 + 3 >= 32)
extern "C" int cn_op_conv1_bordered(const float* x, const float* w9c, const float* bias, void* out, int32_t B, int32_t T, int32_t F,
                                    int32_t C, void* stream) {
    return launch_conv1_bordered_bf16(x, w9c, bias, out, B, T, F, (T - 1) / 2 + 1, (F - 1) / 2 + 1, C, (hipStream_t)stream);
}

// conv front-end of the fp8 engine through the ABI (config 5): conv1 -> e4m3fn image at `img_scale` (bordered) -> conv2 on e4m3
// operands; w2_host fp32 [C][3][3][C] (k = (kh * 3 + kw) * C + ci) is quantised here at the largest power-of-two scale that keeps it
// in range.  img8_out_dev (optional): the bordered image [B][T1 + 2][F1 + 2][C] bytes.  out: bf16 [B * T2 * F2][C], or with
// out8_scale > 0 e4m3fn bytes at that scale (what linear_out's e4m3 form reads)
extern "C" int cn_op_conv_frontend_fp8(const float* x_dev, const float* w1_9c_dev, const float* b1_dev, const float* w2_host,
                                       const float* b2_dev, void* out_dev, void* img8_out_dev, int32_t B, int32_t T, int32_t F,
                                       int32_t C, float img_scale, float out8_scale, float* w_scale_out, void* stream) {
    if (!conv2_f8_applies(C, C)) {
        cn_set_error("cn_op_conv_frontend_fp8: 256 channels only");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int T1 = (T - 1) / 2 + 1, F1 = (F - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1, F2 = (F1 - 1) / 2 + 1;
    std::vector<unsigned char> w8((size_t)C * 9 * C);
    const int lg = pack_conv2_f8(w2_host, C, 9 * C, C, 1, w8.data());
    if (w_scale_out) *w_scale_out = std::ldexp(1.f, lg);
    const int q[4] = {127 - lg, 127 - (int)std::lround(std::log2(img_scale)), 0, 0};
    const size_t img_bytes = (size_t)B * (T1 + 2) * (F1 + 2) * C;
    Scratch sc("cn_op_conv_frontend_fp8", s);
    void* dw = sc.upload(w8.data(), w8.size());
    void* dq = sc.upload(q, 16);
    void* img = sc.alloc(img_bytes);
    if (!sc.ok()) return -2;
    CN_HIP_CHECK(hipMemsetAsync(img, 0xff, img_bytes, s));  // (NaN bytes: the kernel must write every cell, border included)
    int rc = launch_conv1_f8(x_dev, w1_9c_dev, b1_dev, img, B, T, F, T1, F1, C, 1, img_scale, s);
    if (rc == 0) rc = launch_conv2_f8(img, dw, (const int*)dq, b2_dev, out_dev, B, T1, F1, T2, F2, s, out8_scale);
    if (rc == 0 && img8_out_dev) CN_HIP_CHECK(hipMemcpyAsync(img8_out_dev, img, img_bytes, hipMemcpyDeviceToDevice, s));
    return sc.finish(rc);
}

// The split-bf16 engine's conv front-end in the MIX arithmetic through the ABI (conv1.hip MIXP planes + conv2.hip MIX): x fp32 [B][T][F],
// w2_host fp32 [C][3][3][C] (k = (kh * 3 + kw) * C + ci); out_dev: split-bf16 rows [B * T2 * F2][C] (cn_op_convert turns them into fp32);
// img_out_dev (optional): conv1's three bordered planes, 4 bytes per cell of [B][T1 + 2][F1 + 2][C] (half values, l bytes, q bytes)
extern "C" int cn_op_conv_frontend_mix(const float* x_dev, const float* w1_9c_dev, const float* b1_dev, const float* w2_host,
                                       const float* b2_dev, void* out_dev, void* img_out_dev, int32_t B, int32_t T, int32_t F, int32_t C,
                                       void* stream) {
    if (!conv2_mix_applies(CN_PREC_X3, C, C)) {
        cn_set_error("cn_op_conv_frontend_mix: 256 channels only (and not in the half-precision build of the library)");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int T1 = (T - 1) / 2 + 1, F1 = (F - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1, F2 = (F1 - 1) / 2 + 1;
    const size_t n = (size_t)C * 9 * C;
    std::vector<unsigned char> w(4 * n);
    int q[4];
    pack_conv2_mix(w2_host, C, 9 * C, C, 1, w.data(), q);
    const size_t img_bytes = (size_t)B * (T1 + 2) * (F1 + 2) * C * 4;
    Scratch sc("cn_op_conv_frontend_mix", s);
    void* dw = sc.upload(w.data(), w.size());
    void* dq = sc.upload(q, 16);
    void* img = sc.alloc(img_bytes);
    if (!sc.ok()) return -2;
    CN_HIP_CHECK(hipMemsetAsync(img, 0xff, img_bytes, s));  // (NaN bytes: conv1 must write every cell of every plane, border included)
    int rc = launch_conv1_mixplanes(x_dev, w1_9c_dev, b1_dev, img, B, T, F, T1, F1, C, 1, std::ldexp(1.f, MIX_LG_AL), std::ldexp(1.f, MIX_LG_AQ), s);
    if (rc == 0)
        rc = launch_conv2_mix(img, dw, (const unsigned char*)dw + 2 * n, (const unsigned char*)dw + 3 * n, (const int*)dq, b2_dev, out_dev, B, T1, F1,
                              T2, F2, s);
    if (rc == 0 && img_out_dev) CN_HIP_CHECK(hipMemcpyAsync(img_out_dev, img, img_bytes, hipMemcpyDeviceToDevice, s));
    return sc.finish(rc);
}

// linear_out of the fp8 engine through the ABI: a8_dev [M][K] e4m3fn at a_scale (K = 5120), w_host fp32 [256][K] quantised here at
// the largest power-of-two scale in range; out fp32 [M][256] = (a . w^T / (a_scale w_scale) + bias) * out_scale + pe[m % pe_period]
extern "C" int cn_op_linear256_fp8(const void* a8_dev, const float* w_host, const float* bias_dev, float* out_dev, int32_t M, int32_t K,
                                   float a_scale, float out_scale, const float* pe_dev, int32_t pe_period, float* w_scale_out,
                                   void* stream) {
    if (!linear256_f8_applies(256, K)) {
        cn_set_error("cn_op_linear256_fp8: K must be 5120");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)256 * K; ++i) mx = std::max(mx, std::fabs(w_host[i]));
    const int lg = cn_e4m3_exp(mx);
    const float ws = std::ldexp(1.f, lg);
    if (w_scale_out) *w_scale_out = ws;
    std::vector<unsigned char> w8((size_t)256 * K);
    for (size_t i = 0; i < w8.size(); ++i) w8[i] = cn_f32_to_e4m3_host(w_host[i] * ws);
    const int q[4] = {127 - lg, 127 - (int)std::lround(std::log2(a_scale)), 0, 0};
    Scratch sc("cn_op_linear256_fp8", s);
    void* dw = sc.upload(w8.data(), w8.size());
    void* dq = sc.upload(q, 16);
    if (!sc.ok()) return -2;
    return sc.finish(launch_linear256_f8(a8_dev, dw, (const int*)dq, bias_dev, out_dev, M, K, out_scale, pe_dev, pe_period, s));
}

extern "C" int cn_op_conv2(int32_t precision, const void* conv1_out, const void* w_khwc, const float* bias, void* out,
                           int32_t B, int32_t T1, int32_t F1, int32_t C, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_conv2")) < 0) return -1;
    GemmArgs g;
    const int T2 = (T1 - 1) / 2 + 1, F2 = (F1 - 1) / 2 + 1;
    g.A = conv1_out;
    g.W = w_khwc;
    g.bias = bias;
    g.C = out;
    g.ldc = C;
    g.M = B * T2 * F2;
    g.N = C;
    g.K = 9 * C;
    g.epi = CN_EPI_RELU;
    g.conv = 1;
    g.cB = B;
    g.cT1 = T1;
    g.cF1 = F1;
    g.cC = C;
    g.cT2 = T2;
    g.cF2 = F2;
    if (!conv2_dma_applies(precision, C, C)) return launch_gemm(precision, g, (hipStream_t)stream);
    // bf16, 256 channels: the LDS-DMA kernel reads an image with a one-cell zero halo (the model has conv1 write it that
    // way); this test entry pads a copy of the plain image
    const size_t cell = (size_t)C * 2, prow = (size_t)(F1 + 2) * cell;
    Scratch sc("cn_op_conv2", (hipStream_t)stream);
    void* padded = sc.alloc((size_t)B * (T1 + 2) * prow);
    if (!sc.ok()) return -2;
    CN_HIP_CHECK(hipMemsetAsync(padded, 0, (size_t)B * (T1 + 2) * prow, (hipStream_t)stream));
    for (int b = 0; b < B; ++b)
        CN_HIP_CHECK(hipMemcpy2DAsync((unsigned char*)padded + ((size_t)b * (T1 + 2) + 1) * prow + cell, prow,
                                      (const unsigned char*)conv1_out + (size_t)b * T1 * F1 * cell, (size_t)F1 * cell,
                                      (size_t)F1 * cell, T1, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    g.A = padded;
    g.conv_halo = 1;
    return sc.finish(launch_gemm(precision, g, (hipStream_t)stream));
}

// host fp32 [rows][K] -> the elements of internal precision `prec` as the generic kernels read them (fp32 as it is, the 16-bit
// operand, or split-bf16 rows: K % 32 == 0)
static std::vector<unsigned char> host_elems(int prec, const float* w, size_t rows, size_t K) {
    std::vector<unsigned char> out(rows * K * cn_elem_size(prec));
    if (prec == CN_PREC_F32) {
        std::memcpy(out.data(), w, out.size());
    } else if (prec == CN_PREC_BF16) {
        for (size_t i = 0; i < rows * K; ++i) {
            const uint16_t v = cn_host_op16(w[i]);
            std::memcpy(&out[2 * i], &v, 2);
        }
    } else {
        for (size_t r = 0; r < rows; ++r)
            for (size_t c = 0; c < K; ++c) {
                const uint16_t hi = cn_host_op16(w[r * K + c]), lo = cn_host_op16(w[r * K + c] - cn_host_op16_value(hi));
                std::memcpy(&out[r * K * 4 + cn_split_off(c)], &hi, 2);
                std::memcpy(&out[r * K * 4 + cn_split_off(c) + 64], &lo, 2);
            }
    }
    return out;
}

// Every launch form of the subsampling front end from one descriptor (include/cassnat_hip.h, cn_frontend_desc).  Everything that
// would be refused is refused here, before the weights are packed and anything touches the device.
extern "C" int cn_op_frontend_desc(const cn_frontend_desc* d, void* stream) {
    const char* who = "cn_op_frontend_desc";
    auto refuse = [&](const std::string& why) {
        cn_set_error(std::string(who) + ": " + why);
        return -1;
    };
    if (!d) return refuse("null descriptor");
    const int c1 = d->conv1_form, c2 = d->conv2_form, ln = d->linear_form;
    if (c1 < 0 || c1 > CN_FE_CONV1_BF16_MFMA || c2 < 0 || c2 > CN_FE_CONV2_F8 || ln < 0 || ln > CN_FE_LINEAR_F8) return refuse("unknown form");
    if (!c1 && !c2 && !ln) return refuse("no stage selected");
    const int prec = cn_own_precision(d->precision, who);
    if (prec < 0) return -1;
    if (prec != CN_PREC_F32 && prec != CN_PREC_BF16 && prec != CN_PREC_X3) return refuse("precision must be CN_PRECISION_F32, BF16, BF16X3 or F16");
#ifdef CN_OP16_F16
    if (c1 == CN_FE_CONV1_PLANES || c1 == CN_FE_CONV1_MIXPLANES || c1 == CN_FE_CONV1_F8_VALU || c1 == CN_FE_CONV1_F8_MFMA || c2 == CN_FE_CONV2_X3 ||
        c2 == CN_FE_CONV2_MIX || c2 == CN_FE_CONV2_F8 || ln == CN_FE_LINEAR_F8)
        return refuse("the half-precision library has no split-bf16, MIX or e4m3 form");
#endif
    const int B = d->B, T = d->T, F = d->F, C = d->C, halo = d->halo;
    const int T1 = (T - 1) / 2 + 1, F1 = (F - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1, F2 = (F1 - 1) / 2 + 1;
    const bool c1_16 = c1 == CN_FE_CONV1_BF16_MFMA || (c1 == CN_FE_CONV1_PLAIN && prec == CN_PREC_BF16);
    if (c1 || c2) {
        if (B < 1 || T < 1 || F < 1 || C < 8 || C % 8 != 0 || 256 % (C / 8) != 0)
            return refuse("B, T, F >= 1 and a channel count that is a multiple of 8 with C / 8 dividing 256");
        if ((long long)B * (T1 + 2) * (F1 + 2) * C >= (1ll << 31)) return refuse("image beyond 2^31 cells");
        if (halo < 0 || halo > 2) return refuse("halo is 0, 1 or 2");
        if (!d->img) return refuse("null img");
    }
    if (c1) {
        if (!d->x || !d->w9c || !d->bias1) return refuse("conv1 needs x, w9c and bias1");
        const bool mfma = c1 == CN_FE_CONV1_F8_MFMA || c1 == CN_FE_CONV1_BF16_MFMA;
        if (mfma && !conv1_mfma_shape_ok(C, F1)) return refuse("the matrix-core conv1 forms need C == 256 and 32 <= F1 + 2 <= 65");
        if (c1 == CN_FE_CONV1_BF16_MFMA && prec != CN_PREC_BF16) return refuse("the 16-bit matrix-core conv1 form needs the 16-bit precision");
        if (mfma && halo != 1) return refuse("halo 0 / 2 on a matrix-core conv1 form: it writes its border always (halo == 1)");
        if (c1 != CN_FE_CONV1_PLAIN && halo == 0) return refuse("halo 0 on a conv1 form whose image is always bordered");
        if (c1 == CN_FE_CONV1_PLAIN && prec == CN_PREC_X3 && (halo || C % 32 != 0))
            return refuse("the plain split-bf16 image (X3 precision) has no halo form and needs C % 32 == 0");
        if ((c1 == CN_FE_CONV1_F8_VALU || c1 == CN_FE_CONV1_F8_MFMA || c1 == CN_FE_CONV1_MIXPLANES) && !(d->img_scale > 0.f))
            return refuse("img_scale must be positive");
        if (c1 == CN_FE_CONV1_MIXPLANES && !(d->img_scale2 > 0.f)) return refuse("img_scale2 must be positive");
        if (d->n_sub < 0 || d->n_sub > CN_MAX_SUB) return refuse("a rows list holds at most " + std::to_string(CN_MAX_SUB) + " batches");
        if (d->n_sub > 0) {
            if (!d->sub_rows || !d->sub_frames) return refuse("n_sub > 0 needs sub_rows and sub_frames");
            long long sum = 0;
            for (int k = 0; k < d->n_sub; ++k) {
                if (d->sub_rows[k] < 1 || d->sub_frames[k] < 1 || d->sub_frames[k] > T) return refuse("a batch needs rows >= 1 and 1 <= frames <= T");
                sum += d->sub_rows[k];
            }
            if (sum != B) return refuse("the rows list sums to " + std::to_string(sum) + ", not to B = " + std::to_string(B));
        }
    }
    if (c2) {
        if (!d->w2 || !d->bias2 || !d->c2_out) return refuse("conv2 needs w2, bias2 and c2_out");
        if (c2 == CN_FE_CONV2_GENERIC && halo && !conv2_dma_applies(prec, C, C))
            return refuse("a bordered image is read by the 16-bit 256-channel tile kernel only (generic conv2: halo 0)");
        if (c2 == CN_FE_CONV2_GENERIC && prec == CN_PREC_X3 && C % 32 != 0) return refuse("split-bf16 rows need C % 32 == 0");
        if (c2 == CN_FE_CONV2_DMA && !conv2_dma_applies(prec, C, C)) return refuse("the LDS-DMA conv2 form needs the 16-bit precision and C == 256");
        if (c2 == CN_FE_CONV2_X3 && !conv2_x3_applies(CN_PREC_X3, C, C)) return refuse("the X3 conv2 form needs C == 256");
        if (c2 == CN_FE_CONV2_MIX && !conv2_mix_applies(CN_PREC_X3, C, C)) return refuse("the MIX conv2 form needs C == 256");
        if (c2 == CN_FE_CONV2_F8 && !conv2_f8_applies(C, C)) return refuse("the e4m3 conv2 form needs C == 256");
        if (c2 != CN_FE_CONV2_GENERIC && halo == 0) return refuse("halo 0 on a conv2 tile form: it reads a bordered image");
        if (c2 == CN_FE_CONV2_F8 && (!(d->img_scale > 0.f) || d->out8_scale < 0.f)) return refuse("img_scale must be positive, out8_scale >= 0");
        if (c1) {  // what conv1 writes is what conv2 reads
            const bool fits = ((c2 == CN_FE_CONV2_GENERIC && halo == 0) && c1 == CN_FE_CONV1_PLAIN) ||
                              ((c2 == CN_FE_CONV2_DMA || (c2 == CN_FE_CONV2_GENERIC && halo)) && c1_16) ||
                              (c2 == CN_FE_CONV2_X3 && c1 == CN_FE_CONV1_PLANES) || (c2 == CN_FE_CONV2_MIX && c1 == CN_FE_CONV1_MIXPLANES) ||
                              (c2 == CN_FE_CONV2_F8 && (c1 == CN_FE_CONV1_F8_VALU || c1 == CN_FE_CONV1_F8_MFMA));
            if (!fits) return refuse("this conv2 form does not read the image this conv1 form writes");
        }
    }
    if (ln) {
        const int M = d->M, K = d->K;
        if (!d->lin_a || !d->lin_w || !d->lin_bias || !d->lin_out) return refuse("linear needs lin_a, lin_w, lin_bias and lin_out");
        if (M < 1 || K < 1 || d->lda < K || d->pe_period < 1) return refuse("linear needs M, K >= 1, lda >= K and pe_period >= 1");
        if (ln == CN_FE_LINEAR_DMA && !linear256_dma_applies(prec, 256, K)) return refuse("the LDS-DMA linear form needs the 16-bit precision, K % 64 == 0 and K >= 128");
        if (ln == CN_FE_LINEAR_DMA && d->lda % 8 != 0) return refuse("the LDS-DMA linear form needs 16-byte aligned rows (lda % 8 == 0)");
        if (ln == CN_FE_LINEAR_F8 && (!linear256_f8_applies(256, K) || d->lda != K || !(d->a_scale > 0.f))) return refuse("the e4m3 linear form needs lda == K == 5120 and a positive a_scale");
        if (ln == CN_FE_LINEAR_GENERIC && ((prec == CN_PREC_X3 && (K % 32 != 0 || d->lda % 32 != 0)) || K % 8 != 0 || d->lda % 8 != 0))
            return refuse("the generic linear form needs K and lda multiples of 8 (split-bf16: of 32)");
    }
    // ---- pack
    hipStream_t s = (hipStream_t)stream;
    const size_t wn = (size_t)C * 9 * C;
    std::vector<unsigned char> w2p, lwp;
    int q2[4] = {0, 0, 0, 0}, ql[4] = {0, 0, 0, 0};
    if (c2 == CN_FE_CONV2_GENERIC || c2 == CN_FE_CONV2_DMA) {
        w2p = host_elems(prec, d->w2, C, (size_t)9 * C);
    } else if (c2 == CN_FE_CONV2_X3) {  // two [C][9 C] planes: the hi halves, then the lo halves (weights.hip, put_hi_lo)
        w2p.resize(4 * wn);
        for (size_t e = 0; e < wn; ++e) {
            const uint16_t hi = cn_host_op16(d->w2[e]), lo = cn_host_op16(d->w2[e] - cn_host_op16_value(hi));
            std::memcpy(&w2p[2 * e], &hi, 2);
            std::memcpy(&w2p[2 * wn + 2 * e], &lo, 2);
        }
    } else if (c2 == CN_FE_CONV2_MIX) {
        w2p.resize(4 * wn);
        pack_conv2_mix(d->w2, C, 9 * C, C, 1, w2p.data(), q2);
    } else if (c2 == CN_FE_CONV2_F8) {
        w2p.resize(wn);
        const int lg = pack_conv2_f8(d->w2, C, 9 * C, C, 1, w2p.data());
        q2[0] = 127 - lg;
        q2[1] = 127 - (int)std::lround(std::log2(d->img_scale));
    }
    if (ln == CN_FE_LINEAR_F8) {
        float mx = 0.f;
        for (size_t i = 0; i < (size_t)256 * d->K; ++i) mx = std::max(mx, std::fabs(d->lin_w[i]));
        const int lg = cn_e4m3_exp(mx);
        lwp.resize((size_t)256 * d->K);
        for (size_t i = 0; i < lwp.size(); ++i) lwp[i] = cn_f32_to_e4m3_host(d->lin_w[i] * std::ldexp(1.f, lg));
        ql[0] = 127 - lg;
        ql[1] = 127 - (int)std::lround(std::log2(d->a_scale));
    } else if (ln) {
        lwp = host_elems(prec, d->lin_w, 256, (size_t)d->K);
    }
    if (d->q8_out) {
        std::memcpy(d->q8_out, q2, 16);
        std::memcpy(d->q8_out + 4, ql, 16);
    }
    Scratch sc(who, s);
    const unsigned char* dw2 = c2 ? (const unsigned char*)sc.upload(w2p.data(), w2p.size()) : nullptr;
    const void* dlw = ln ? sc.upload(lwp.data(), lwp.size()) : nullptr;
    const int* dq2 = c2 ? (const int*)sc.upload(q2, 16) : nullptr;
    const int* dql = ln ? (const int*)sc.upload(ql, 16) : nullptr;
    UttMeta* meta = (c1 && d->n_sub > 0) ? (UttMeta*)sc.alloc((size_t)B * sizeof(UttMeta)) : nullptr;
    if (!sc.ok()) return -2;
    // ---- launch
    int rc = 0;
    if (meta) {
        SubList subs;
        std::memset(&subs, 0, sizeof(subs));
        subs.n = d->n_sub;
        for (int k = 0; k < d->n_sub; ++k) {
            subs.rows[k] = d->sub_rows[k];
            subs.frames[k] = d->sub_frames[k];
        }
        rc = launch_expand_meta(subs, meta, B, s);
        if (rc == 0 && d->meta_out) CN_HIP_CHECK(hipMemcpyAsync(d->meta_out, meta, (size_t)B * sizeof(UttMeta), hipMemcpyDeviceToDevice, s));
    }
    if (rc == 0 && c1 == CN_FE_CONV1_PLAIN) rc = launch_conv1(prec, d->x, d->w9c, d->bias1, d->img, B, T, F, T1, F1, C, halo, s, meta);
    if (rc == 0 && c1 == CN_FE_CONV1_PLANES) rc = launch_conv1_planes(d->x, d->w9c, d->bias1, d->img, B, T, F, T1, F1, C, halo, s, meta);
    if (rc == 0 && c1 == CN_FE_CONV1_MIXPLANES)
        rc = launch_conv1_mixplanes(d->x, d->w9c, d->bias1, d->img, B, T, F, T1, F1, C, halo, d->img_scale, d->img_scale2, s, meta);
    if (rc == 0 && (c1 == CN_FE_CONV1_F8_VALU || c1 == CN_FE_CONV1_F8_MFMA))
        rc = launch_conv1_f8_form(c1 == CN_FE_CONV1_F8_MFMA, d->x, d->w9c, d->bias1, d->img, B, T, F, T1, F1, C, halo, d->img_scale, s, meta);
    if (rc == 0 && c1 == CN_FE_CONV1_BF16_MFMA) rc = launch_conv1_bordered_bf16(d->x, d->w9c, d->bias1, d->img, B, T, F, T1, F1, C, s, meta);
    if (rc == 0 && c2 == CN_FE_CONV2_GENERIC) {
        GemmArgs g;
        g.A = d->img;
        g.conv_halo = halo ? 1 : 0;
        g.W = dw2;
        g.bias = d->bias2;
        g.C = d->c2_out;
        g.ldc = C;
        g.M = B * T2 * F2;
        g.N = C;
        g.K = 9 * C;
        g.epi = CN_EPI_RELU;
        g.conv = 1;
        g.cB = B;
        g.cT1 = T1;
        g.cF1 = F1;
        g.cC = C;
        g.cT2 = T2;
        g.cF2 = F2;
        rc = launch_gemm(prec, g, s);
    }
    if (rc == 0 && c2 == CN_FE_CONV2_DMA) rc = launch_conv2_dma(d->img, dw2, d->bias2, d->c2_out, B, T1, F1, T2, F2, s);
    if (rc == 0 && c2 == CN_FE_CONV2_X3) {
        const size_t plane = (size_t)B * (T1 + 2) * (F1 + 2) * C * 2;
        rc = launch_conv2_x3(d->img, (const unsigned char*)d->img + plane, dw2, dw2 + 2 * wn, d->bias2, d->c2_out, B, T1, F1, T2, F2, s);
    }
    if (rc == 0 && c2 == CN_FE_CONV2_MIX) rc = launch_conv2_mix(d->img, dw2, dw2 + 2 * wn, dw2 + 3 * wn, dq2, d->bias2, d->c2_out, B, T1, F1, T2, F2, s);
    if (rc == 0 && c2 == CN_FE_CONV2_F8) rc = launch_conv2_f8(d->img, dw2, dq2, d->bias2, d->c2_out, B, T1, F1, T2, F2, s, d->out8_scale);
    if (rc == 0 && ln == CN_FE_LINEAR_GENERIC) {
        GemmArgs g;
        g.A = d->lin_a;
        g.lda = d->lda;
        g.W = dlw;
        g.bias = d->lin_bias;
        g.C = d->lin_out;
        g.ldc = 256;
        g.c_f32 = 1;
        g.M = d->M;
        g.N = 256;
        g.K = d->K;
        g.epi = CN_EPI_EMBED;
        g.pe = d->pe;
        g.pe_period = d->pe_period;
        g.scale = d->scale;
        rc = launch_gemm(prec, g, s);
    }
    if (rc == 0 && ln == CN_FE_LINEAR_DMA)
        rc = launch_linear256_dma(d->lin_a, d->lda, dlw, d->lin_bias, d->lin_out, d->M, d->K, d->scale, d->pe, d->pe_period, s);
    if (rc == 0 && ln == CN_FE_LINEAR_F8)
        rc = launch_linear256_f8(d->lin_a, dlw, dql, d->lin_bias, d->lin_out, d->M, d->K, d->scale, d->pe, d->pe_period, s);
    return sc.finish(rc);
}
extern "C" int32_t cn_frontend_desc_size(void) { return (int32_t)sizeof(cn_frontend_desc); }

extern "C" int cn_op_layernorm(int32_t precision, const float* x, const float* a2, const float* b2, void* y, int32_t M,
                               int32_t d, float eps, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_layernorm")) < 0) return -1;
    return launch_layernorm(precision, x, a2, b2, y, 0, M, d, eps, (hipStream_t)stream);
}

// ---- the conformer convolution module's kernels (conformer.hip), one at a time
// the kernels index rows of d elements and an utterance's L x d image with int: refuse what would not fit
static int conv_module_dims(const char* who, int precision, long long rows, long long row_len, int d, const char* what) {
    if (precision != CN_PREC_F32 && precision != CN_PREC_BF16 && precision != CN_PREC_X3) {
        cn_set_error(std::string(who) + ": precision must be F32, BF16 (F16 in the half-precision build) or BF16X3");
        return -1;
    }
    if (precision == CN_PREC_X3 && d % 32 != 0) {
        cn_set_error(std::string(who) + ": split-bf16 (bf16x3) rows are groups of 32 elements: d % 32 != 0 has no layout");
        return -1;
    }
    if (row_len * d > 0x7fffffffLL || rows * row_len > 0x7fffffffLL || rows * row_len * d >= (1LL << 39)) {
        cn_set_error(std::string(who) + ": " + what + " exceeds the kernels' int arithmetic (2^31 - 1; all elements together: 2^39)");
        return -1;
    }
    return 0;
}

extern "C" int cn_op_glu(int32_t precision, const void* in, void* out, int32_t M, int32_t d, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_glu")) < 0) return -1;
    if (!in || !out) {
        cn_set_error("cn_op_glu: null pointer (in, out)");
        return -1;
    }
    if (M < 1 || d < 1) {
        cn_set_error("cn_op_glu: M and d must be >= 1");
        return -1;
    }
    // (the input row holds 2 d elements)
    CN_TRY(conv_module_dims("cn_op_glu", precision, 1, 2LL * M, d, "M * 2d"));
    return launch_glu(precision, in, out, M, d, (hipStream_t)stream);
}

extern "C" int cn_op_dwconv(int32_t precision, const void* x, const float* w, const float* bias, float* y, int32_t B, int32_t L,
                            int32_t d, int32_t k, int32_t form, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_dwconv")) < 0) return -1;
    if (!x || !w || !bias || !y) {
        cn_set_error("cn_op_dwconv: null pointer (x, w, bias, y)");
        return -1;
    }
    if (B < 1 || L < 1 || d < 1 || k < 1) {
        cn_set_error("cn_op_dwconv: B, L, d and k must be >= 1");
        return -1;
    }
    if (form != 0 && form != 1) {
        cn_set_error("cn_op_dwconv: form must be 0 (the launcher's choice) or 1 (the naive kernel)");
        return -1;
    }
    CN_TRY(conv_module_dims("cn_op_dwconv", precision, B, L, d, "L * d (or B * L)"));
    if ((long long)d * k > 0x7fffffffLL || (long long)L + k > 0x7fffffffLL) {
        cn_set_error("cn_op_dwconv: d * k and L + k exceed the kernels' int arithmetic (<= 2^31 - 1)");
        return -1;
    }
    return launch_dwconv(precision, x, w, bias, y, B, L, d, k, form, (hipStream_t)stream);
}

extern "C" int cn_op_groupnorm_swish(int32_t precision, const float* x, double* stats, const float* gw, const float* gb, void* out,
                                     int32_t B, int32_t L, int32_t d, float eps, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_groupnorm_swish")) < 0) return -1;
    if (!x || !stats || !gw || !gb || !out) {
        cn_set_error("cn_op_groupnorm_swish: null pointer (x, stats, gw, gb, out)");
        return -1;
    }
    if (B < 1 || L < 1 || d < 1) {
        cn_set_error("cn_op_groupnorm_swish: B, L and d must be >= 1");
        return -1;
    }
    CN_TRY(conv_module_dims("cn_op_groupnorm_swish", precision, B, L, d, "L * d (or B * L)"));
    return launch_groupnorm_swish(precision, x, stats, gw, gb, out, B, L, d, eps, (hipStream_t)stream);
}

extern "C" int cn_op_attention(int32_t precision, const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V,
                               int32_t ldv, void* O, int32_t ldo, int32_t B, int32_t H, int32_t Lq, int32_t Lk,
                               const uint8_t* keymask, const int32_t* klen, const int32_t* intervals, int32_t iv_stride,
                               int32_t causal, float scale, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_attention")) < 0) return -1;
    AttnArgs a;
    a.Q = Q;
    a.K = K;
    a.V = V;
    a.O = O;
    a.ldq = ldq;
    a.ldk = ldk;
    a.ldv = ldv;
    a.ldo = ldo;
    a.B = B;
    a.H = H;
    a.Lq = Lq;
    a.Lk = Lk;
    a.keymask = keymask;
    a.klen = klen;
    a.intervals = intervals;
    a.iv_stride = iv_stride;
    a.causal = causal;
    a.scale = scale;
    int rc = launch_attention(precision, a, (hipStream_t)stream);
    if (rc == 0 && cn_exp_env("CASSNAT_ATTN_STAMPS")) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)attention_print_stamps();
    }
    return rc;
}

static int op_attention_desc(const char* who, int32_t precision, const cn_attn_desc* d, const int32_t* row_off, int32_t kv_packed,
                             void* stream) {
    if ((precision = cn_own_precision(precision, who)) < 0) return -1;
    if (!d) {
        cn_set_error(std::string(who) + ": null descriptor");
        return -1;
    }
    AttnArgs a;
    a.row_off = row_off;
    a.kv_packed = kv_packed;
    a.Q = d->Q;
    a.K = d->K;
    a.V = d->V;
    a.O = d->O;
    a.ldq = d->ldq;
    a.ldk = d->ldk;
    a.ldv = d->ldv;
    a.ldo = d->ldo;
    a.B = d->B;
    a.H = d->H;
    a.Lq = d->Lq;
    a.Lk = d->Lk;
    a.keymask = d->keymask;
    a.kv_mod = d->kv_mod;
    a.kv_index = d->kv_index;
    a.klen = d->klen;
    a.kcap = d->kcap;
    a.kcap_stride = d->kcap_stride;
    a.q_blocked = d->q_blocked;
    a.kv_blocked = d->kv_blocked;
    a.q_col = d->q_col;
    a.k_col = d->k_col;
    a.v_col = d->v_col;
    a.q_n = d->q_n;
    a.kv_n = d->kv_n;
    a.o_blocked = d->o_blocked;
    a.intervals = d->intervals;
    a.iv_stride = d->iv_stride;
    a.causal = d->causal;
    a.scale = d->scale;
    a.rel_pos = d->rel_pos;
    a.rel_u = d->rel_u;
    a.rel_v = d->rel_v;
    a.rel_R = d->rel_R;
    a.ld_pos = d->ld_pos;
    return launch_attention(precision, a, (hipStream_t)stream);
}

extern "C" int cn_op_attention_desc(int32_t precision, const cn_attn_desc* d, void* stream) {
    return op_attention_desc("cn_op_attention_desc", precision, d, nullptr, 0, stream);
}

// The projecting form (attention.hip, PROJ) on a caller's LNn(x): the Q|K|V projection is packed as the tail of a chain stream
// (pack_chain, as cn_op_chain packs it on every call) and the kernel reads its units and biases from there
extern "C" int cn_op_attention_proj(int32_t precision, const cn_attn_desc* d, const void* y_dev, const float* wt_host,
                                    const float* bt_host, void* stream) {
    if ((precision = cn_own_precision(precision, "cn_op_attention_proj")) < 0) return -1;
    if (!d || !y_dev || !wt_host || !bt_host) {
        cn_set_error("cn_op_attention_proj: null argument");
        return -1;
    }
    if (precision != CN_PREC_BF16) {
        cn_set_error("cn_op_attention_proj: the projecting form exists for the 16-bit kernels");
        return -1;
    }
    ChainWeights w;
    w.wt = wt_host;
    w.bt = bt_host;
    w.tail_n = 768;
    std::vector<uint16_t> hs(chain_stream_units(0, 0, 768) * (CHAIN_UNIT_BYTES / 2));
    std::vector<float> ht(CHAIN_TAB_FLOATS);
    pack_chain(w, hs.data(), ht.data());
    Scratch sc("cn_op_attention_proj", (hipStream_t)stream);
    const void* ds = sc.upload(hs.data(), hs.size() * 2);
    const float* dt = (const float*)sc.upload(ht.data(), ht.size() * 4);
    if (!sc.ok()) return -2;
    AttnArgs a;
    a.O = d->O;
    a.ldo = d->ldo;
    a.B = d->B;
    a.H = d->H;
    a.Lq = d->Lq;
    a.Lk = d->Lk;
    a.keymask = d->keymask;
    a.kv_mod = d->kv_mod;
    a.kv_index = d->kv_index;
    a.klen = d->klen;
    a.kcap = d->kcap;
    a.kcap_stride = d->kcap_stride;
    a.o_blocked = d->o_blocked;
    a.intervals = d->intervals;
    a.iv_stride = d->iv_stride;
    a.causal = d->causal;
    a.scale = d->scale;
    a.rel_pos = d->rel_pos;
    a.proj_y = y_dev;
    a.proj_w = ds;
    a.proj_b = dt + CHAIN_TAB_BT;
    return sc.finish(launch_attention(precision, a, (hipStream_t)stream));
}

extern "C" int cn_op_attention_packed(int32_t precision, const cn_attn_desc* d, const int32_t* row_off_dev, int32_t kv_packed,
                                      void* stream) {
    if (!row_off_dev) {
        cn_set_error("cn_op_attention_packed: null row_off");
        return -1;
    }
    return op_attention_desc("cn_op_attention_packed", precision, d, row_off_dev, kv_packed, stream);
}

extern "C" int cn_op_row_plan(const int32_t* ylen_dev, int32_t B, int32_t U, int32_t hyp_stride, int32_t sub, const int32_t* utt_meta_dev,
                              const int32_t* ymax_dev, int32_t* row_off_dev, void* stream) {
    static_assert(sizeof(UttMeta) == 4 * sizeof(int32_t), "cn_op_row_plan: utt_meta is [B][4] int32");
    if (!ylen_dev || !row_off_dev || B < 1 || U < 0 || sub < 0) {
        cn_set_error("cn_op_row_plan: null argument or B < 1");
        return -1;
    }
    return launch_row_plan(ylen_dev, B, U, hyp_stride, sub, reinterpret_cast<const UttMeta*>(utt_meta_dev), ymax_dev, row_off_dev,
                           (hipStream_t)stream);
}

extern "C" int32_t cn_attn_desc_size(void) { return (int32_t)sizeof(cn_attn_desc); }

extern "C" int cn_op_logsoftmax_argmax(float* logits, int32_t M, int32_t V, int32_t* arg, float* maxlp,
                                       int32_t write_logp, void* stream) {
    return launch_logsoftmax_argmax(logits, M, V, V, arg, maxlp, write_logp, (hipStream_t)stream);
}

// Every form of the alignment kernel from one descriptor (include/cassnat_hip.h, cn_align_desc): everything that would be refused is
// refused here, before anything touches the caller's buffers.
static int op_ctc_align_desc(const char* who, const cn_align_desc* d, void* stream) {
    static_assert(sizeof(UttMeta) == 4 * sizeof(int32_t), "cn_align_desc: utt_meta is [B][4] int32");
    auto refuse = [&](const char* what) {
        cn_set_error(std::string(who) + ": " + what);
        return -1;
    };
    if (!d) return refuse("null descriptor");
    if (!d->best || !d->keymask || !d->size_ratio) return refuse("null best, keymask or size_ratio");
    if (!d->shift || !d->src_size || !d->ylen || !d->ymax || !d->intervals) return refuse("null shift, src_size, ylen, ymax or intervals");
    if (d->B < 1 || d->Tp < 1) return refuse("B and Tp must be >= 1");
    if (d->src_mod < 0 || d->left < 0 || d->right < 0) return refuse("src_mod, left and right must not be negative");
    hipStream_t s = (hipStream_t)stream;
    if (d->utt_meta) {  // the kernel indexes its LDS rows and the key mask by the records' T': check them where they can be read
        const int n = d->src_mod > 0 ? std::min(d->src_mod, d->B) : d->B;
        std::vector<UttMeta> meta((size_t)n);
        CN_HIP_CHECK(hipMemcpyAsync(meta.data(), d->utt_meta, (size_t)n * sizeof(UttMeta), hipMemcpyDeviceToHost, s));
        CN_HIP_CHECK(hipStreamSynchronize(s));
        for (const UttMeta& m : meta)
            if (m.tp < 1 || m.tp > d->Tp) return refuse("a utt_meta record's T' lies outside 1 .. Tp");
    }
    AlignArgs a;
    a.best = d->best;
    a.keymask = d->keymask;
    a.size_ratio = d->size_ratio;
    a.B = d->B;
    a.Tp = d->Tp;
    a.blank = d->blank;
    a.left = d->left;
    a.right = d->right;
    a.src_mod = d->src_mod;
    a.shift = d->shift;
    a.src_size = d->src_size;
    a.ylen = d->ylen;
    a.ymax = d->ymax;
    a.intervals = d->intervals;
    a.raw_path = d->raw_path;
    a.ylen_in = d->ylen_in;
    a.utt_meta = reinterpret_cast<const UttMeta*>(d->utt_meta);
    a.no_trigger = d->no_trigger;
    return launch_ctc_align(a, s);
}

extern "C" int cn_op_ctc_align_desc(const cn_align_desc* d, void* stream) { return op_ctc_align_desc("cn_op_ctc_align_desc", d, stream); }
extern "C" int32_t cn_align_desc_size(void) { return (int32_t)sizeof(cn_align_desc); }

// cn_op_ctc_align: the descriptor of the plain form
extern "C" int cn_op_ctc_align(const int32_t* best, const uint8_t* keymask, const float* size_ratio, int32_t B,
                               int32_t Tp, int32_t blank, int32_t left, int32_t right, int32_t* shift,
                               int32_t* src_size, int32_t* ylen, int32_t* ymax, int32_t* intervals, void* stream) {
    cn_align_desc d = {};
    d.best = best;
    d.keymask = keymask;
    d.size_ratio = size_ratio;
    d.B = B;
    d.Tp = Tp;
    d.blank = blank;
    d.left = left;
    d.right = right;
    d.shift = shift;
    d.src_size = src_size;
    d.ylen = ylen;
    d.ymax = ymax;
    d.intervals = intervals;
    return op_ctc_align_desc("cn_op_ctc_align", &d, stream);
}

// The search kernel (ctc_beam.hip) alone on given log-posteriors and given pruned labels: the check (`who` in its message; a's own
// mandatory descriptor null: desc_missing), which refuses before the GPU is touched, the back-pointers' scratch, the launch.
static int op_ctc_beam(const char* who, bool desc_missing, CtcSearchArgs a, void* stream) {
    if (!a.ng && !a.bias && !a.merge && a.B <= 0) return 0;
    const std::string bad = desc_missing ? "null argument" : ctc_search_check(a, false);
    if (!bad.empty()) {
        cn_set_error(std::string(who) + ": " + bad);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    Scratch sc(who, s);
    a.hist_parent = (unsigned char*)sc.alloc((size_t)a.B * a.Tp * a.W);
    a.hist_tok = (int*)sc.alloc((size_t)a.B * a.Tp * a.W * 4);
    if (!sc.ok()) return -2;
    return sc.finish(launch_ctc_beam(a, s));
}

// the two kernels of decode_type ctc_only / ctc_att on given log-posteriors (test entries; all pointers device)
extern "C" int cn_op_ctc_prefix_beam(const float* logp, const float* size_ratio, int32_t B, int32_t Tp, int32_t V, int32_t beam,
                                     int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp, int32_t hyp_cap,
                                     int32_t* hyp_len, double* score, double* p_blk, double* p_nblk, int32_t* nbeam, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t M = (size_t)B * Tp;
    const int P = pruning > 0 ? pruning : 1;
    Scratch sc("cn_op_ctc_prefix_beam", s);
    int* top_idx = (int*)sc.alloc(M * P * 4);
    float* top_val = (float*)sc.alloc(M * P * 4);
    if (!sc.ok()) return -2;
    const int rc = pruning > 0 ? launch_topk(logp, (int)M, V, V, pruning, top_idx, top_val, s) : 0;
    if (rc != 0) return sc.finish(rc);
    return op_ctc_beam("cn_op_ctc_prefix_beam", false,
                       ctc_search_args(ctc_beam_args(logp, top_idx, size_ratio, B, Tp, V, beam, pruning, blank, length_penalty,
                                                     ctc_beam_out(hyp, hyp_cap, hyp_len, score, nullptr, p_blk, p_nblk, nbeam))),
                       stream);
}

extern "C" int cn_op_ctc_viterbi(const float* logp, const uint8_t* keymask, const float* size_ratio, const int32_t* labels,
                                 const int32_t* label_len, int32_t B, int32_t Tp, int32_t V, int32_t ld, int32_t ymax, int32_t blank,
                                 int32_t* out_path, void* stream) {
    if (!logp || !keymask || !size_ratio || !labels || !label_len || !out_path) {
        cn_set_error("cn_op_ctc_viterbi: null pointer (logp, keymask, size_ratio, labels, label_len, out_path)");
        return -1;
    }
    if (B < 1 || Tp < 1 || V < 1 || ymax < 1 || ld < ymax) {
        cn_set_error("cn_op_ctc_viterbi: B, Tp, V and ymax must be >= 1, ld >= ymax");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    Scratch sc("cn_op_ctc_viterbi", s);
    unsigned char* bp = (unsigned char*)sc.alloc((size_t)B * Tp * (2 * (size_t)ymax + 1));
    if (!sc.ok()) return -2;
    ViterbiArgs v;
    v.logp = logp;
    v.keymask = keymask;
    v.size_ratio = size_ratio;
    v.labels = labels;
    v.label_len = label_len;
    v.B = B;
    v.Tp = Tp;
    v.V = V;
    v.ld = ld;
    v.ymax = ymax;
    v.blank = blank;
    v.bp = bp;
    v.out_path = out_path;
    return sc.finish(launch_ctc_viterbi(v, s));
}

// the forced alignment with spans and confidences on given log-posteriors (include/cassnat_hip_ctc_times.h; all pointers device)
extern "C" int cn_op_ctc_token_times(const float* logp_dev, const int32_t* frames_dev, const int32_t* labels_dev, int32_t ld,
                                     const int32_t* label_len_dev, int32_t B, int32_t Tp, int32_t V, int32_t blank, int64_t bp_lds_limit,
                                     int32_t* start_dev, int32_t* end_dev, float* conf_dev, double* score_dev, int32_t* status_dev,
                                     void* stream) {
    CtcTimesArgs a;
    a.logp = logp_dev, a.frames = frames_dev, a.labels = labels_dev, a.label_len = label_len_dev;
    a.B = B, a.Tp = Tp, a.V = V, a.ld = ld, a.blank = blank;
    a.start = start_dev, a.end = end_dev, a.conf = conf_dev, a.score = score_dev, a.status = status_dev;
    const std::string bad = ct_check(a);  // (before the scratch is sized from these numbers)
    if (!bad.empty()) {
        cn_set_error("cn_op_ctc_token_times: " + bad);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    Scratch sc("cn_op_ctc_token_times", s);
    if (const size_t need = ct_scratch_bytes(B, Tp, ld, bp_lds_limit)) a.bp = (unsigned long long*)sc.alloc(need);
    if (!sc.ok()) return -2;
    return sc.finish(launch_ctc_token_times(a, bp_lds_limit, s));
}

// the weighted edit alignment of id sequences (include/cassnat_hip_score.h; all pointers device)
extern "C" int cn_op_edit_align(const int32_t* ref_dev, int64_t ref_total, const int64_t* ref_begin_dev, const int32_t* ref_len_dev,
                                const int32_t* hyp_dev, int64_t hyp_total, const int64_t* hyp_begin_dev, const int32_t* hyp_len_dev, int32_t N,
                                int32_t max_ref, int32_t max_hyp, int32_t c_sub, int32_t c_ins, int32_t c_del, int64_t bp_lds_limit,
                                int32_t* cost_dev, int32_t* counts_dev, int32_t* path_len_dev, uint8_t* ops_dev, int64_t ops_total,
                                const int64_t* ops_begin_dev, void* stream) {
    EditArgs a;
    a.ref = ref_dev, a.ref_begin = ref_begin_dev, a.ref_len = ref_len_dev, a.hyp = hyp_dev, a.hyp_begin = hyp_begin_dev, a.hyp_len = hyp_len_dev;
    a.ops_begin = ops_begin_dev, a.ref_total = ref_total, a.hyp_total = hyp_total, a.ops_total = ops_total;
    a.N = N, a.max_ref = max_ref, a.max_hyp = max_hyp, a.c_sub = c_sub, a.c_ins = c_ins, a.c_del = c_del;
    a.cost = cost_dev, a.counts = counts_dev, a.path_len = path_len_dev, a.ops = ops_dev;
    const std::string bad = ea_check(a);  // (before the scratch is sized from these numbers)
    if (!bad.empty()) {
        cn_set_error("cn_op_edit_align: " + bad);
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    Scratch sc("cn_op_edit_align", s);
    if (const size_t need = ea_scratch_bytes(N, max_ref, max_hyp, bp_lds_limit)) a.bp = (unsigned long long*)sc.alloc(need);
    if (!sc.ok()) return -2;
    return sc.finish(launch_edit_align(a, bp_lds_limit, s));
}

static int op_greedy_pack(const char* who, const int32_t* tok, const float* val, const int32_t* ylen, int32_t B, int32_t U, int32_t sos,
                          int32_t hyp_stride, int32_t* hyp, int32_t* hyp_len, double* score, int32_t sub, const int32_t* utt_meta_dev,
                          const int32_t* ymax_dev, const int32_t* row_off_dev, void* stream) {
    if (!tok || !val || !ylen || !hyp || !hyp_len || !score) {
        cn_set_error(std::string(who) + ": null pointer (tok, val, ylen, hyp, hyp_len, score)");
        return -1;
    }
    if (B < 1 || U < 1 || hyp_stride < 1 || sub < 0) {
        cn_set_error(std::string(who) + ": B, U and hyp_stride must be >= 1, sub >= 0");
        return -1;
    }
    // device-side records the kernel indexes by are read back and checked, as cn_op_ctc_align_desc checks its records' T': a batch
    // inside the call; offsets that keep every utterance's rows inside the B * U rows tok / val hold (what a plan of <= U rows each gives)
    hipStream_t s = (hipStream_t)stream;
    if (utt_meta_dev) {
        std::vector<UttMeta> meta((size_t)B);
        CN_HIP_CHECK(hipMemcpyAsync(meta.data(), utt_meta_dev, (size_t)B * sizeof(UttMeta), hipMemcpyDeviceToHost, s));
        CN_HIP_CHECK(hipStreamSynchronize(s));
        for (const UttMeta& m : meta)
            if (m.sub_lo < 0 || m.sub_hi < m.sub_lo || m.sub_hi > B) {
                cn_set_error(std::string(who) + ": a utt_meta record's batch lies outside 0 .. B");
                return -1;
            }
    }
    if (row_off_dev) {
        std::vector<int32_t> off((size_t)B + 1);
        CN_HIP_CHECK(hipMemcpyAsync(off.data(), row_off_dev, ((size_t)B + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        CN_HIP_CHECK(hipStreamSynchronize(s));
        for (int b = 0; b <= B; ++b)
            if (off[b] < 0 || (long long)off[b] > (long long)b * U || (b > 0 && off[b] < off[b - 1])) {
                cn_set_error(std::string(who) + ": row_off must be non-decreasing with 0 <= row_off[b] <= b * U");
                return -1;
            }
    }
    return launch_greedy_pack(tok, val, ylen, B, U, sos, hyp_stride, hyp, hyp_len, score, (hipStream_t)stream, sub,
                              reinterpret_cast<const UttMeta*>(utt_meta_dev), ymax_dev, row_off_dev);
}

extern "C" int cn_op_greedy_pack(const int32_t* tok, const float* val, const int32_t* ylen, int32_t B, int32_t U,
                                 int32_t sos, int32_t hyp_stride, int32_t* hyp, int32_t* hyp_len, double* score,
                                 void* stream) {
    return op_greedy_pack("cn_op_greedy_pack", tok, val, ylen, B, U, sos, hyp_stride, hyp, hyp_len, score, 0, nullptr, nullptr, nullptr, stream);
}

extern "C" int cn_op_greedy_pack_rows(const int32_t* tok, const float* val, const int32_t* ylen, int32_t B, int32_t U, int32_t sos,
                                      int32_t hyp_stride, int32_t* hyp, int32_t* hyp_len, double* score, int32_t sub,
                                      const int32_t* utt_meta_dev, const int32_t* ymax_dev, const int32_t* row_off_dev, void* stream) {
    return op_greedy_pack("cn_op_greedy_pack_rows", tok, val, ylen, B, U, sos, hyp_stride, hyp, hyp_len, score, sub, utt_meta_dev, ymax_dev,
                          row_off_dev, stream);
}

extern "C" int cn_op_ctc_collapse(const int32_t* best, const uint8_t* keymask, int32_t B, int32_t Tp, int32_t sos, int32_t pad, int32_t ld,
                                  int32_t* tgt, int32_t* len, int32_t* keylen, int32_t* maxlen, void* stream) {
    if (!best || !keymask || !tgt || !len || !keylen || !maxlen) {
        cn_set_error("cn_op_ctc_collapse: null pointer (best, keymask, tgt, len, keylen, maxlen)");
        return -1;
    }
    return launch_ctc_collapse(best, keymask, B, Tp, sos, pad, ld, tgt, len, keylen, maxlen, (hipStream_t)stream);
}

extern "C" int cn_op_esa_paths(const int32_t* top2_idx, const float* top2_val, const uint8_t* select, float threshold, int32_t* best,
                               int32_t M, int32_t n, void* stream) {
    if (!top2_idx || !top2_val || !best) {
        cn_set_error("cn_op_esa_paths: null pointer (top2_idx, top2_val, best)");
        return -1;
    }
    if (M < 1 || n < 1) {
        cn_set_error("cn_op_esa_paths: M and n must be >= 1");
        return -1;
    }
    return launch_esa_paths(top2_idx, top2_val, select, threshold, best, M, n, (hipStream_t)stream);
}

extern "C" int cn_op_keymask(const float* feats, int32_t B, int32_t T, int32_t F, int32_t Tp, int32_t stride, float padding, uint8_t* keymask,
                             void* stream) {
    if (!feats || !keymask) {
        cn_set_error("cn_op_keymask: null pointer (feats, keymask)");
        return -1;
    }
    if (B < 1 || T < 1 || F < 1 || Tp < 1 || stride < 1) {
        cn_set_error("cn_op_keymask: B, T, F, Tp and stride must be >= 1");
        return -1;
    }
    if ((long long)B * Tp > 0x7fffffffLL || (long long)stride * (Tp - 1) > 0x7fffffffLL) {
        cn_set_error("cn_op_keymask: B * Tp and stride * (Tp - 1) exceed the kernel's int arithmetic (<= 2^31 - 1)");
        return -1;
    }
    return launch_keymask(feats, B, T, F, Tp, stride, padding, keymask, (hipStream_t)stream);
}

extern "C" int cn_op_expand_meta(const int32_t* rows_host, const int32_t* frames_host, int32_t n, int32_t* utt_meta_dev, int32_t B,
                                 void* stream) {
    static_assert(sizeof(UttMeta) == 4 * sizeof(int32_t), "cn_op_expand_meta: utt_meta is [B][4] int32");
    if (!rows_host || !frames_host || !utt_meta_dev) {
        cn_set_error("cn_op_expand_meta: null pointer (rows, frames, utt_meta)");
        return -1;
    }
    if (n < 1 || n > CN_MAX_SUB) {
        cn_set_error("cn_op_expand_meta: a rows list holds 1 .. " + std::to_string(CN_MAX_SUB) + " batches");
        return -1;
    }
    if (B < 1) {
        cn_set_error("cn_op_expand_meta: B must be >= 1");
        return -1;
    }
    SubList subs;
    std::memset(&subs, 0, sizeof(subs));
    subs.n = n;
    for (int k = 0; k < n; ++k) {
        if (rows_host[k] < 1 || frames_host[k] < 1) {
            cn_set_error("cn_op_expand_meta: a batch needs rows >= 1 and frames >= 1");
            return -1;
        }
        subs.rows[k] = rows_host[k];
        subs.frames[k] = frames_host[k];
    }
    return launch_expand_meta(subs, reinterpret_cast<UttMeta*>(utt_meta_dev), B, (hipStream_t)stream);
}

extern "C" int cn_op_topk(const float* logp, int32_t M, int32_t V, int32_t k, int32_t* idx, float* val, void* stream) {
    return launch_topk(logp, M, V, V, k, idx, val, (hipStream_t)stream);
}

// fp8 product through the ABI (config 5): A bf16 on the device is quantised at a_scale, W (HOST fp32 [N][K]) at the largest
// power-of-two scale that fits e4m3fn (as cn_model_finalize does); C = relu?(A_q . W_q^T / scales + bias), fp32 [M][N]
extern "C" int cn_op_gemm_fp8(const void* a_bf16_dev, int32_t lda, const float* w_host, const float* bias_dev, float* c_dev,
                              int32_t M, int32_t N, int32_t K, float a_scale, int32_t relu, float* w_scale_out, void* stream) {
    if (M < 1 || N < 1 || K < 128 || K % 128 != 0) {
        cn_set_error("cn_op_gemm_fp8: K must be a positive multiple of 128");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)N * K; ++i) mx = std::max(mx, std::fabs(w_host[i]));
    const float ws = std::ldexp(1.f, cn_e4m3_exp(mx));
    if (w_scale_out) *w_scale_out = ws;
    std::vector<unsigned char> w8((size_t)N * K);
    for (size_t i = 0; i < w8.size(); ++i) w8[i] = cn_f32_to_e4m3_host(w_host[i] * ws);
    Scratch sc("cn_op_gemm_fp8", s);
    void* dw = sc.upload(w8.data(), w8.size());
    void* da = sc.alloc((size_t)M * K);
    if (!sc.ok()) return -2;
    int rc = launch_quantize_fp8(a_bf16_dev, lda, da, M, K, a_scale, s);
    if (rc == 0) {
        GemmArgs g;
        g.A = da;
        g.lda = K;
        g.W = dw;
        g.bias = bias_dev;
        g.C = c_dev;
        g.ldc = N;
        g.c_f32 = 1;
        g.M = M;
        g.N = N;
        g.K = K;
        g.epi = relu ? CN_EPI_RELU : 0;
        g.ab_fp8 = 1;
        g.acc_scale = 1.f / (a_scale * ws);
        rc = launch_gemm(CN_PREC_BF16, g, s);
    }
    return sc.finish(rc);
}

extern "C" int cn_op_cmvn(float* feats_dev, const int32_t* len_dev, const double* mean_dev, const double* std_dev, int32_t B, int32_t T,
                          int32_t F, void* stream) {
    if (!feats_dev || !len_dev || !mean_dev || !std_dev) {
        cn_set_error("cn_op_cmvn: null argument");
        return -1;
    }
    return launch_cmvn(feats_dev, len_dev, mean_dev, std_dev, B, T, F, (hipStream_t)stream);
}

// Host side of the packed reader: n byte ranges (an utterance's rows inside the memory map of an archive) copied back to back into a
// page-locked staging buffer in ONE call - ctypes releases the GIL for its duration, so the decode pipelines' host threads copy side
// by side (numpy's slice assignment holds it: two threads took turns, 5 ms a turn).  threads > 1: the ranges are dealt over that
// many std::threads in equal byte shares (--load_data_workers on this path).
extern "C" int cn_host_gather(void* dst, const uint64_t* src_ptrs, const uint64_t* dst_offsets, const uint64_t* nbytes, int32_t n,
                              int32_t threads) {
    if (!dst || !src_ptrs || !dst_offsets || !nbytes || n < 0) {
        cn_set_error("cn_host_gather: null argument");
        return -1;
    }
    auto run = [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i)
            memcpy(static_cast<unsigned char*>(dst) + dst_offsets[i], reinterpret_cast<const void*>(src_ptrs[i]), nbytes[i]);
    };
    const int nt = std::max(1, std::min<int>(threads, n));
    if (nt == 1) {
        run(0, n);
        return 0;
    }
    uint64_t total = 0;
    for (int i = 0; i < n; ++i) total += nbytes[i];
    std::vector<std::thread> pool;
    int lo = 0;
    uint64_t acc = 0;
    for (int t = 0; t < nt; ++t) {
        int hi = lo;
        const uint64_t want = total * (uint64_t)(t + 1) / (uint64_t)nt;
        while (hi < n && (t + 1 == nt || acc + nbytes[hi] <= want || hi == lo)) acc += nbytes[hi++];
        if (t + 1 < nt) pool.emplace_back(run, lo, hi);
        else run(lo, hi);
        lo = hi;
    }
    for (auto& th : pool) th.join();
    return 0;
}

// Host side of the FLAC reader: the exact frame index of a stream's audio bytes (flac_format.h: one linear pass, every frame's CRC-16
// checked); GIL-free like the gather, the loader's workers and the pipelines' threads run it side by side.
extern "C" int cn_host_flac_index(const void* audio, int64_t nbytes, int32_t rate, int32_t channels, int32_t bits, int32_t* out,
                                  int64_t capacity, int64_t* frames, int64_t* samples, int64_t* bad_offset) {
    if (!audio || nbytes < 0 || !frames || !samples || !bad_offset || capacity < 0) {
        cn_set_error("cn_host_flac_index: null argument");
        return -1;
    }
    const int rc = flac_index(static_cast<const uint8_t*>(audio), nbytes, rate, channels, bits, out, capacity, frames, samples, bad_offset);
    if (rc == FLAC_INDEX_NO_CHAIN)
        cn_set_error("cn_host_flac_index: no chain of frames with matching CRCs reaches the end: it breaks at byte offset " +
                     std::to_string(*bad_offset));
    else if (rc == FLAC_INDEX_FORMAT)
        cn_set_error("cn_host_flac_index: the frame at byte offset " + std::to_string(*bad_offset) +
                     " has another sample rate, channel count or sample size than STREAMINFO");
    else if (rc == FLAC_INDEX_CAPACITY)
        cn_set_error("cn_host_flac_index: more frames than the output holds");
    else if (rc == FLAC_INDEX_RANGE)
        cn_set_error("cn_host_flac_index: offsets or sample counts beyond 2^31 - 1");
    return rc;
}

extern "C" int32_t cn_host_flac_crc16(const void* data, int64_t nbytes) {
    return data && nbytes > 0 ? (int32_t)flac_crc16(static_cast<const uint8_t*>(data), nbytes) : 0;
}

extern "C" int64_t cn_flac_frame_words(int32_t channels, int32_t block_size) { return flac_frame_words(channels, block_size); }

extern "C" int64_t cn_flac_scratch_bytes(int32_t frames, int64_t frame_words) { return flac_scratch_bytes(frames, frame_words); }

extern "C" int cn_op_flac_decode(const void* staged_dev, int64_t staged_bytes, const int32_t* table_dev, int32_t frames, const int32_t* utt_dev,
                                 int32_t utts, int32_t max_channels, int64_t frame_words, void* pcm_dev, int64_t pcm_bytes,
                                 int32_t* status_dev, void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (!staged_dev || !table_dev || !utt_dev || !pcm_dev || !status_dev) {
        cn_set_error("cn_op_flac_decode: null argument");
        return -1;
    }
    if (frames < 1 || utts < 1 || max_channels < 1 || max_channels > 8 || staged_bytes < 0 || pcm_bytes < 0 ||
        frame_words < flac_frame_words(1, 1) || frame_words > flac_frame_words(8, 65536)) {
        cn_set_error("cn_op_flac_decode: need frames, utts >= 1, 1 <= max_channels <= 8 and frame_words of at least one sample");
        return -1;
    }
    if (((size_t)pcm_dev & 1) || ((size_t)scratch_dev & 3)) {
        cn_set_error("cn_op_flac_decode: the PCM buffer must be 2-byte, the scratch 4-byte aligned");
        return -1;
    }
    const int64_t need = flac_scratch_bytes(frames, frame_words);
    if (scratch_dev) {  // the caller's scratch (the packed reader keeps one per slot): nothing is allocated, nothing waited for
        if (scratch_bytes < need) {
            cn_set_error("cn_op_flac_decode: the scratch holds " + std::to_string(scratch_bytes) + " bytes, the pass needs " + std::to_string(need));
            return -1;
        }
        return launch_flac_decode(static_cast<const unsigned char*>(staged_dev), staged_bytes, table_dev, frames, utt_dev, utts, max_channels,
                                  frame_words, static_cast<unsigned char*>(pcm_dev), pcm_bytes, status_dev, static_cast<int*>(scratch_dev),
                                  (hipStream_t)stream);
    }
    Scratch sc("cn_op_flac_decode", (hipStream_t)stream);
    int* scratch = static_cast<int*>(sc.alloc((size_t)need));
    if (!sc.ok()) return -2;
    return sc.finish(launch_flac_decode(static_cast<const unsigned char*>(staged_dev), staged_bytes, table_dev, frames, utt_dev, utts,
                                        max_channels, frame_words, static_cast<unsigned char*>(pcm_dev), pcm_bytes, status_dev, scratch,
                                        (hipStream_t)stream));
}

extern "C" int cn_op_unpack_rows(const float* packed_dev, const int32_t* off_dev, const int32_t* len_dev, float* out_dev, int32_t rows,
                                 int32_t T, int32_t F, float pad, const double* mean_dev, const double* std_dev, void* stream) {
    if (!packed_dev || !off_dev || !len_dev || !out_dev || (!mean_dev) != (!std_dev)) {
        cn_set_error("cn_op_unpack_rows: null argument (mean and std come together)");
        return -1;
    }
    return launch_unpack_rows(packed_dev, off_dev, len_dev, out_dev, rows, T, F, pad, mean_dev, std_dev, (hipStream_t)stream);
}

extern "C" int cn_op_unpack_compressed(const void* staged_dev, const int32_t* off_dev, const int32_t* len_dev, const int32_t* kind_dev,
                                       float* out_dev, int32_t rows, int32_t T, int32_t F, float pad, const double* mean_dev,
                                       const double* std_dev, void* stream) {
    if (!staged_dev || !off_dev || !len_dev || !kind_dev || !out_dev || (!mean_dev) != (!std_dev)) {
        cn_set_error("cn_op_unpack_compressed: null argument (mean and std come together)");
        return -1;
    }
    if (((size_t)staged_dev) & 15) {
        cn_set_error("cn_op_unpack_compressed: the staging buffer must start on a 16-byte boundary");
        return -1;
    }
    return launch_unpack_compressed(static_cast<const unsigned char*>(staged_dev), off_dev, len_dev, kind_dev, out_dev, rows, T, F, pad,
                                    mean_dev, std_dev, (hipStream_t)stream);
}

extern "C" int cn_op_splice_rows(const float* src_dev, const int32_t* off_dev, const int32_t* len_dev, float* out_dev, int32_t rows,
                                 int32_t T_out, int32_t F0, int32_t left, int32_t right, int32_t skip, float pad, const double* mean_dev,
                                 const double* std_dev, void* stream) {
    if (!src_dev || !off_dev || !len_dev || !out_dev || (!mean_dev) != (!std_dev)) {
        cn_set_error("cn_op_splice_rows: null argument (mean and std come together)");
        return -1;
    }
    return launch_splice_rows(src_dev, off_dev, len_dev, out_dev, rows, T_out, F0, left, right, skip, pad, mean_dev, std_dev,
                              (hipStream_t)stream);
}

extern "C" int cn_op_quantize_fp8(const void* src_bf16_dev, int32_t ld, void* dst_dev, int32_t M, int32_t K, float scale,
                                  void* stream) {
    return launch_quantize_fp8(src_bf16_dev, ld, dst_dev, M, K, scale, (hipStream_t)stream);
}

extern "C" int cn_op_logsoftmax_topk(const float* logits, int32_t M, int32_t V, float temperature, int32_t k, int32_t* idx,
                                     float* val, void* stream) {
    return launch_logsoftmax_topk(logits, M, V, V, temperature, k, idx, val, (hipStream_t)stream);
}

extern "C" int cn_op_logsoftmax_fuse_topk(const float* att, const float* lm, int32_t M, int32_t V, float temperature, float w,
                                          int32_t k, int32_t* idx, float* val, void* stream) {
    if (M < 0 || V < 1 || (M > 0 && (!att || !lm || !idx || !val))) {
        cn_set_error("cn_op_logsoftmax_fuse_topk: bad argument");
        return -1;
    }
    return launch_logsoftmax_fuse_topk(att, lm, M, V, V, temperature, w, k, idx, val, (hipStream_t)stream);
}

extern "C" int cn_op_logsoftmax_gather(const float* logits, int32_t M, int32_t V, const int32_t* cand, int32_t k, float* out,
                                       void* stream) {
    if (M < 0 || V < 1 || (M > 0 && (!logits || !cand || !out))) {
        cn_set_error("cn_op_logsoftmax_gather: bad argument");
        return -1;
    }
    return launch_logsoftmax_gather(logits, M, V, V, cand, k, out, (hipStream_t)stream);
}

// ---- kernel-test entries of the AST beam search's step kernels (ast.hip)
// what the two gather-attention entries share: the precision, the common shape checks (min_ldq: 3d behind the fused Q | K | V
// projection, d for plain queries; `keys`: the entry's name of its key count) and the common fields of the arguments
static int gather_args_of(GatherArgs& a, int32_t& precision, const char* who, const char* keys, int32_t nkeys, int32_t min_ldq,
                          const void* q, int32_t ldq, void* k, void* v, void* o, int32_t ldo, int32_t n, int32_t H, int32_t d,
                          int32_t table_stride, float scale) {
    if ((precision = cn_own_precision(precision, who)) < 0) return -1;
    if (precision != CN_PREC_F32 && precision != CN_PREC_BF16 && precision != CN_PREC_X3) {
        cn_set_error(std::string(who) + ": precision must be F32, BF16 (F16 in the half-precision build) or BF16X3");
        return -1;
    }
    if (n < 0 || H < 1 || H > 16 || d != 64 * H || nkeys < 1 || ldo < d || ldq < min_ldq || !q || !k || !v || (n > 0 && !o)) {
        cn_set_error(std::string(who) + ": need 1 <= H <= 16, d = 64 * H, " + keys + " >= 1, ldo >= d, ldq >= " +
                     (min_ldq == d ? "d" : "3d") + " and the q / k / v / o arrays");
        return -1;
    }
    a.q = q;
    a.ldq = ldq;
    a.k = k;
    a.v = v;
    a.o = o;
    a.ldo = ldo;
    a.n = n;
    a.H = H;
    a.d = d;
    a.table_stride = table_stride;
    a.scale = scale;
    return 0;
}

extern "C" int cn_op_ast_gather_attn(int32_t precision, int32_t mode, const void* q, int32_t ldq, void* k, void* v, void* o,
                                     int32_t ldo, int32_t n, int32_t H, int32_t nkeys, int32_t slots, int32_t d, int32_t table_stride,
                                     const int32_t* anc, const uint8_t* keyok, const int32_t* utt, const uint8_t* keymask, float scale,
                                     int32_t append_pos, void* stream) {
    if (mode != 0 && mode != 1) {
        cn_set_error("cn_op_ast_gather_attn: mode must be 0 (cache) or 1 (source memory)");
        return -1;
    }
    GatherAttnArgs a;
    CN_TRY(gather_args_of(a, precision, "cn_op_ast_gather_attn", "nkeys", nkeys, mode == 0 ? 3 * d : d, q, ldq, k, v, o, ldo, n, H, d,
                          table_stride, scale));
    if (mode == 0 && (slots < n || table_stride < nkeys || append_pos < -1 || append_pos >= nkeys || !anc || !keyok)) {
        cn_set_error("cn_op_ast_gather_attn: mode 0 needs slots >= n, table_stride >= nkeys, -1 <= append_pos < nkeys, anc and keyok");
        return -1;
    }
    if (mode == 1 && (!utt || !keymask)) {
        cn_set_error("cn_op_ast_gather_attn: mode 1 needs utt and keymask");
        return -1;
    }
    a.nkeys = nkeys;
    a.slots = slots;
    a.anc = anc;
    a.keyok = keyok;
    a.utt = utt;
    a.keymask = keymask;
    a.append_pos = mode == 0 ? append_pos : -1;
    return launch_ast_gather_attn(precision, mode, a, (hipStream_t)stream);
}

extern "C" int cn_op_ast_gather_attn_rows(int32_t precision, const void* q, int32_t ldq, void* k, void* v, void* o, int32_t ldo, int32_t n,
                                          int32_t H, int32_t d, int32_t table_stride, int32_t max_keys, const int32_t* rowid,
                                          const int32_t* pos, const int32_t* stay, float scale, void* stream) {
    GatherRowsArgs a;
    CN_TRY(gather_args_of(a, precision, "cn_op_ast_gather_attn_rows", "max_keys", max_keys, 3 * d, q, ldq, k, v, o, ldo, n, H, d,
                          table_stride, scale));
    if (table_stride < max_keys || !rowid || !pos || !stay) {
        cn_set_error("cn_op_ast_gather_attn_rows: need table_stride >= max_keys and the rowid, pos and stay tables");
        return -1;
    }
    a.max_keys = max_keys;
    a.rowid = rowid;
    a.pos = pos;
    a.stay = stay;
    return launch_ast_gather_attn_rows(precision, a, (hipStream_t)stream);
}

extern "C" int cn_op_ast_ctc_prepare(float* logp, const uint8_t* keymask, float* r0, int32_t B, int32_t Tp, int32_t V, int32_t blank,
                                     void* stream) {
    if (B < 1 || Tp < 1 || V < 1 || blank < 0 || blank >= V || !logp || !keymask || !r0) {
        cn_set_error("cn_op_ast_ctc_prepare: need B, Tp, V >= 1, 0 <= blank < V and non-null buffers");
        return -1;
    }
    return launch_ast_ctc_prepare(logp, keymask, r0, B, Tp, V, blank, (hipStream_t)stream);
}

extern "C" int cn_op_ast_ctc_prefix(const float* logp, const float* r0, const float* r_prev, float* r_new, const int32_t* utt,
                                    const int32_t* last_tok, const int32_t* cand, const int32_t* prev_ref, float* score, int32_t n,
                                    int32_t K, int32_t Tp, int32_t V, int32_t blank, int32_t eos, int32_t out_len, void* stream) {
    if (n < 0 || K < 1 || Tp < 1 || V < 1 || blank < 0 || blank >= V || out_len < 0 || out_len > Tp ||
        (n > 0 && (!logp || !r0 || !r_new || !utt || !last_tok || !cand || !prev_ref || !score))) {
        cn_set_error("cn_op_ast_ctc_prefix: need n >= 0, K, Tp, V >= 1, 0 <= blank < V, 0 <= out_len <= Tp and non-null buffers");
        return -1;
    }
    CtcPrefixArgs a;
    a.logp = logp;
    a.r0 = r0;
    a.r_prev = r_prev;
    a.r_new = r_new;
    a.utt = utt;
    a.last_tok = last_tok;
    a.cand = cand;
    a.prev_ref = prev_ref;
    a.score = score;
    a.n = n;
    a.K = K;
    a.Tp = Tp;
    a.V = V;
    a.blank = blank;
    a.eos = eos;
    a.out_len = out_len;
    return launch_ast_ctc_prefix(a, (hipStream_t)stream);
}

// the nine arrays every token-level beam keeps (kernels.h: BeamTables); a null one is refused with the entry's own words
static int beam_tables_of(BeamTables& st, int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0, uint8_t* keyok1,
                          double* score0, double* score1, int32_t* cur_tok, const std::string& null_error) {
    const void* all[] = {tok0, tok1, anc0, anc1, keyok0, keyok1, score0, score1, cur_tok};
    for (const void* ptr : all)
        if (!ptr) {
            cn_set_error(null_error);
            return -1;
        }
    st.tok[0] = tok0;
    st.tok[1] = tok1;
    st.anc[0] = anc0;
    st.anc[1] = anc1;
    st.keyok[0] = keyok0;
    st.keyok[1] = keyok1;
    st.score[0] = score0;
    st.score[1] = score1;
    st.cur_tok = cur_tok;
    return 0;
}

static int ast_beam_state_of(AstBeamState& st, int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0,
                             uint8_t* keyok1, int32_t* len0, int32_t* len1, double* score0, double* score1, int32_t* valid0,
                             int32_t* valid1, int32_t* ctc_ref0, int32_t* ctc_ref1, float* ctc_prev0, float* ctc_prev1, int32_t* cur_tok,
                             int32_t* utt, int32_t* live, const char* who) {
    const std::string null_error = std::string(who) + ": null state array";
    CN_TRY(beam_tables_of(st, tok0, tok1, anc0, anc1, keyok0, keyok1, score0, score1, cur_tok, null_error));
    const void* all[] = {len0, len1, valid0, valid1, ctc_ref0, ctc_ref1, ctc_prev0, ctc_prev1, utt, live};
    for (const void* ptr : all)
        if (!ptr) {
            cn_set_error(null_error);
            return -1;
        }
    st.len[0] = len0;
    st.len[1] = len1;
    st.valid[0] = valid0;
    st.valid[1] = valid1;
    st.ctc_ref[0] = ctc_ref0;
    st.ctc_ref[1] = ctc_ref1;
    st.ctc_prev[0] = ctc_prev0;
    st.ctc_prev[1] = ctc_prev1;
    st.utt = utt;
    st.live = live;
    return 0;
}

extern "C" int cn_op_ast_beam_init(int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0, uint8_t* keyok1,
                                   int32_t* len0, int32_t* len1, double* score0, double* score1, int32_t* valid0, int32_t* valid1,
                                   int32_t* ctc_ref0, int32_t* ctc_ref1, float* ctc_prev0, float* ctc_prev1, int32_t* cur_tok, int32_t* utt,
                                   int32_t* live, int32_t cur, int32_t B, int32_t bw, int32_t L, int32_t sos, int32_t pad, void* stream) {
    if (B < 1 || bw < 1 || bw > 32 || L < 1 || (cur != 0 && cur != 1)) {
        cn_set_error("cn_op_ast_beam_init: need B >= 1, 1 <= beam_width <= 32, L >= 1 and cur 0 or 1");
        return -1;
    }
    AstBeamState st;
    CN_TRY(ast_beam_state_of(st, tok0, tok1, anc0, anc1, keyok0, keyok1, len0, len1, score0, score1, valid0, valid1, ctc_ref0, ctc_ref1,
                             ctc_prev0, ctc_prev1, cur_tok, utt, live, "cn_op_ast_beam_init"));
    return launch_ast_beam_init(st, cur, B, bw, L, sos, pad, (hipStream_t)stream);
}

extern "C" int cn_op_ast_beam_update(int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0, uint8_t* keyok1,
                                     int32_t* len0, int32_t* len1, double* score0, double* score1, int32_t* valid0, int32_t* valid1,
                                     int32_t* ctc_ref0, int32_t* ctc_ref1, float* ctc_prev0, float* ctc_prev1, int32_t* cur_tok,
                                     int32_t* utt, int32_t* live, const int32_t* idx, const float* att, const float* ctc, const float* lm,
                                     int32_t cur, int32_t pos, int32_t bw, int32_t K, int32_t L, int32_t eos, int32_t sos, int32_t pad,
                                     int32_t use_ctc, int32_t use_lp, int32_t use_lm, float w, float u, float lw, double lp, int32_t B,
                                     void* stream) {
    if (B < 1 || bw < 1 || bw > 32 || K < bw || K > 32 || L < 1 || (cur != 0 && cur != 1) || !idx || !att || (use_ctc && !ctc) ||
        (use_ctc && use_lm && !lm)) {
        cn_set_error("cn_op_ast_beam_update: need B >= 1, 1 <= beam_width <= K <= 32, L >= 1, cur 0 or 1 and the step's arrays");
        return -1;
    }
    AstBeamState st;
    CN_TRY(ast_beam_state_of(st, tok0, tok1, anc0, anc1, keyok0, keyok1, len0, len1, score0, score1, valid0, valid1, ctc_ref0, ctc_ref1,
                             ctc_prev0, ctc_prev1, cur_tok, utt, live, "cn_op_ast_beam_update"));
    AstBeamStep q;
    q.idx = idx;
    q.att = att;
    q.ctc = ctc;
    q.lm = lm;
    q.cur = cur;
    q.pos = pos;
    q.bw = bw;
    q.K = K;
    q.L = L;
    q.eos = eos;
    q.sos = sos;
    q.pad = pad;
    q.use_ctc = use_ctc;
    q.use_lp = use_lp;
    q.use_lm = use_lm;
    q.w = w;
    q.u = u;
    q.lw = lw;
    q.lp = lp;
    return launch_ast_beam_update(st, q, B, (hipStream_t)stream);
}

// natlm.hip one kernel at a time (cn_nat_lm_finish runs them inside its loop); every array is the caller's, on the device
extern "C" int cn_op_nat_lm_fuse_topk(const float* att, const float* lm, const int32_t* last, const int32_t* zlen, int32_t B, int32_t U,
                                      int32_t V, int32_t bw, int32_t step, float w, int32_t k, int32_t* idx, float* val, void* stream) {
    if (B < 1 || V < 1 || !att || !lm || !idx || !val) {
        cn_set_error("cn_op_nat_lm_fuse_topk: bad argument");
        return -1;
    }
    NatFuseArgs a;
    a.att = att;
    a.lm = lm;
    a.last = last;
    a.zlen = zlen;
    a.idx = idx;
    a.val = val;
    a.U = U;
    a.V = V;
    a.bw = bw;
    a.step = step;
    a.k = k;
    a.w = w;
    return launch_nat_lm_fuse_topk(a, B * bw, (hipStream_t)stream);
}

extern "C" int cn_op_nat_beam_update(int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0, uint8_t* keyok1,
                                     double* score0, double* score1, int32_t* cur_tok, const int32_t* idx, const float* val,
                                     const int32_t* last, int32_t cur, int32_t step, int32_t bw, int32_t L, int32_t pad, int32_t use_lp,
                                     double lp, int32_t B, void* stream) {
    NatBeamState st;
    CN_TRY(beam_tables_of(st, tok0, tok1, anc0, anc1, keyok0, keyok1, score0, score1, cur_tok, "cn_op_nat_beam_update: null array"));
    if (!idx || !val || !last) {
        cn_set_error("cn_op_nat_beam_update: null array");
        return -1;
    }
    NatBeamStep q;
    q.idx = idx;
    q.val = val;
    q.last = last;
    q.cur = cur;
    q.step = step;
    q.bw = bw;
    q.L = L;
    q.pad = pad;
    q.use_lp = use_lp;
    q.lp = lp;
    return launch_nat_beam_update(st, q, B, (hipStream_t)stream);
}

// ctc_lm.hip one kernel at a time (cn_ctc_beam_lm runs them inside its loop); every array is the caller's, on the device
extern "C" int cn_op_ctc_lm_frame(double* pb, double* pnb, double* sctc, double* slm, int32_t* len, int32_t* last, int32_t* nb, int32_t* tok,
                                  int32_t* pos, int32_t* parent, int32_t* stay, const int32_t* rowid_cur, int32_t* rowid_nxt,
                                  uint8_t* hist_parent, int32_t* hist_tok, const float* logp, const int32_t* top_idx, const float* lmrow,
                                  const int32_t* frames, const int32_t* count, int32_t B, int32_t Tp, int32_t V, int32_t W, int32_t P,
                                  int32_t blank, int32_t sos, int32_t iter, int32_t Lt, int32_t hist_stride, double lp, double lm_weight,
                                  void* stream) {
    const void* all[] = {pb, pnb, sctc, slm, len, last, nb, tok, pos, parent, stay, rowid_cur, rowid_nxt, hist_parent, hist_tok, logp,
                         top_idx, lmrow, frames, count};
    for (const void* ptr : all)
        if (!ptr) {
            cn_set_error("cn_op_ctc_lm_frame: null array");
            return -1;
        }
    if (B < 1 || V < 1 || sos < 0 || sos >= V) {
        cn_set_error("cn_op_ctc_lm_frame: need B >= 1 and sos inside the vocabulary");
        return -1;
    }
    CtcLmState st;
    st.pb = pb;
    st.pnb = pnb;
    st.sctc = sctc;
    st.slm = slm;
    st.len = len;
    st.last = last;
    st.nb = nb;
    st.tok = tok;
    st.pos = pos;
    st.parent = parent;
    st.stay = stay;
    st.rowid[iter & 1] = const_cast<int32_t*>(rowid_cur);
    st.rowid[(iter & 1) ^ 1] = rowid_nxt;
    CtcLmFrame a;
    static_cast<CtcBeamArgs&>(a) = ctc_beam_args(logp, top_idx, nullptr, B, Tp, V, W, P, blank, lp, CtcBeamOut());
    a.hist_parent = hist_parent, a.hist_tok = hist_tok;
    a.lmrow = lmrow, a.frames = frames, a.count = count;
    a.sos = sos, a.iter = iter, a.Lt = Lt, a.hist_stride = hist_stride, a.lm_weight = lm_weight;
    return launch_ctc_lm_frame(st, a, (hipStream_t)stream);
}

extern "C" int cn_op_ctc_lm_rows(const float* fresh, const float* prv, float* nxt, const int32_t* parent, const int32_t* stay,
                                 const int32_t* count, int32_t iter, int32_t slots, int32_t W, int32_t V, void* stream) {
    if (!fresh || !prv || !nxt || !parent || !stay) {
        cn_set_error("cn_op_ctc_lm_rows: null array");
        return -1;
    }
    return launch_ctc_lm_rows(fresh, prv, nxt, parent, stay, count, iter, slots, W, V, (hipStream_t)stream);
}

// op_ctc_beam with a policy, on the caller's pruned labels (cn_ctc_beam_ngram / _bias / _merged run the same kernels behind the encoder)
extern "C" int cn_op_ctc_ngram_beam(const cn_ngram_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                                    int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, double lm_scale,
                                    int32_t blank, int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm,
                                    double* p_blk, double* p_nblk, int32_t* nbeam, void* stream) {
    return op_ctc_beam("cn_op_ctc_ngram_beam", !desc,
                       ctc_search_args(ctc_beam_args(logp, top_idx, size_ratio, B, Tp, V, beam, pruning, blank, length_penalty,
                                                     ctc_beam_out(hyp, hyp_cap, hyp_len, score, score_lm, p_blk, p_nblk, nbeam)),
                                       desc, lm_scale),
                       stream);
}

extern "C" int cn_op_ctc_bias_beam(const cn_bias_desc* desc, const float* logp, const int32_t* top_idx, const float* size_ratio, int32_t B,
                                   int32_t Tp, int32_t V, int32_t beam, int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp,
                                   int32_t hyp_cap, int32_t* hyp_len, double* score, double* score_lm, double* p_blk, double* p_nblk,
                                   int32_t* nbeam, void* stream) {
    return op_ctc_beam("cn_op_ctc_bias_beam", !desc,
                       ctc_search_args(ctc_beam_args(logp, top_idx, size_ratio, B, Tp, V, beam, pruning, blank, length_penalty,
                                                     ctc_beam_out(hyp, hyp_cap, hyp_len, score, score_lm, p_blk, p_nblk, nbeam)),
                                       nullptr, 0.0, desc),
                       stream);
}

// (merging by prefix, include/cassnat_hip_ctc_merge.h: both descriptors may be null)
extern "C" int cn_op_ctc_merged_beam(const cn_ngram_desc* ngram_desc, double lm_scale, const cn_bias_desc* bias_desc, const float* logp,
                                     const int32_t* top_idx, const float* size_ratio, int32_t B, int32_t Tp, int32_t V, int32_t beam,
                                     int32_t pruning, double length_penalty, int32_t blank, int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len,
                                     double* score, double* score_lm, double* p_blk, double* p_nblk, int32_t* nbeam, void* stream) {
    return op_ctc_beam("cn_op_ctc_merged_beam", false,
                       ctc_search_args(ctc_beam_args(logp, top_idx, size_ratio, B, Tp, V, beam, pruning, blank, length_penalty,
                                                     ctc_beam_out(hyp, hyp_cap, hyp_len, score, score_lm, p_blk, p_nblk, nbeam)),
                                       ngram_desc, lm_scale, bias_desc, true),
                       stream);
}

extern "C" int cn_op_ffn_fused(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host,
                               const float* b1_dev, const float* w2_host, const float* b2_dev, const float* nln_a_dev,
                               const float* nln_b_dev, void* xn_out_dev, int32_t M, int32_t dff, float eps,
                               int32_t nslice, void* stream) {
    return cn_op_ffn_fused_act(x_dev, ln_a_dev, ln_b_dev, w1_host, b1_dev, w2_host, b2_dev, nln_a_dev, nln_b_dev, xn_out_dev, M, dff, eps,
                               nslice, CN_ACT_RELU, stream);
}

extern "C" int cn_op_ffn_fused_act(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host,
                                   const float* b1_dev, const float* w2_host, const float* b2_dev, const float* nln_a_dev,
                                   const float* nln_b_dev, void* xn_out_dev, int32_t M, int32_t dff, float eps,
                                   int32_t nslice, int32_t act, void* stream) {
    if (act != CN_ACT_RELU && act != CN_ACT_SWISH) {
        cn_set_error("cn_op_ffn_fused_act: act must be CN_ACT_RELU or CN_ACT_SWISH");
        return -1;
    }
    if (dff <= 0 || dff % 128 != 0 || dff > 2048) {
        cn_set_error("cn_op_ffn_fused: d_ff must be a positive multiple of 128, at most 2048");
        return -1;
    }
    const size_t n = (size_t)dff * 256;
    std::vector<uint16_t> h1(n), h2(n);
    pack_ffn_w1(w1_host, dff, h1.data());
    pack_ffn_w2(w2_host, dff, h2.data());
    Scratch sc("cn_op_ffn_fused", (hipStream_t)stream);
    FfnFusedArgs a;
    a.x = x_dev;
    a.ln_a = ln_a_dev;
    a.ln_b = ln_b_dev;
    a.w1p = sc.upload(h1.data(), n * 2);
    a.b1 = b1_dev;
    a.w2p = sc.upload(h2.data(), n * 2);
    a.b2 = b2_dev;
    a.nln_a = nln_a_dev;
    a.nln_b = nln_b_dev;
    a.xn_out = xn_out_dev;
    a.M = M;
    a.d = 256;
    a.dff = dff;
    a.eps = eps;
    a.act = act == CN_ACT_SWISH ? FF_ACT_SWISH : FF_ACT_RELU;
    if (nslice > 1) {  // d_ff split + reduce (the decode-step form)
        a.nslice = nslice;
        a.partial = (float*)sc.alloc((size_t)nslice * M * 256 * 4);
    }
    if (!sc.ok()) return -2;
    int rc = launch_ffn_fused(a, (hipStream_t)stream);
    if (rc == 0 && nslice > 1)
        rc = launch_ffn_reduce(x_dev, a.partial, nslice, b2_dev, nln_a_dev, nln_b_dev, xn_out_dev, M, eps, (hipStream_t)stream);
    return sc.finish(rc);
}

// the same sublayer in the split-bf16 precision (fused_x3.hip); xn_out_dev: split-bf16 [M][256] or NULL
extern "C" int cn_op_ffn_x3(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host, const float* b1_dev,
                            const float* w2_host, const float* b2_dev, const float* nln_a_dev, const float* nln_b_dev,
                            void* xn_out_dev, int32_t M, int32_t dff, float eps, int32_t mix, void* stream) {
    return cn_op_ffn_x3_act(x_dev, ln_a_dev, ln_b_dev, w1_host, b1_dev, w2_host, b2_dev, nln_a_dev, nln_b_dev, xn_out_dev, M, dff, eps, mix,
                            CN_ACT_RELU, stream);
}

extern "C" int cn_op_ffn_x3_act(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host, const float* b1_dev,
                                const float* w2_host, const float* b2_dev, const float* nln_a_dev, const float* nln_b_dev,
                                void* xn_out_dev, int32_t M, int32_t dff, float eps, int32_t mix, int32_t act, void* stream) {
    if (act != CN_ACT_RELU && (act != CN_ACT_SWISH || mix)) {
        cn_set_error("cn_op_ffn_x3_act: act must be CN_ACT_RELU, or CN_ACT_SWISH without the mixed arithmetic");
        return -1;
    }
    if (!ffn_x3_applies(256, dff)) {
        cn_set_error("cn_op_ffn_x3: d_ff must be a positive multiple of 128, at most 2048");
        return -1;
    }
    const size_t bytes = ffn_x3_stream_bytes(dff);
    std::vector<uint16_t> h(bytes / 2);
    pack_ffn_x3(w1_host, w2_host, dff, h.data(), mix != 0);
    Scratch sc("cn_op_ffn_x3", (hipStream_t)stream);
    FfnX3Args a;
    a.x = x_dev;
    a.ln_a = ln_a_dev;
    a.ln_b = ln_b_dev;
    a.wst = sc.upload(h.data(), bytes);
    a.mix = mix != 0;
    a.b1 = b1_dev;
    a.b2 = b2_dev;
    a.nln_a = nln_a_dev;
    a.nln_b = nln_b_dev;
    a.xn_out = xn_out_dev;
    a.M = M;
    a.d = 256;
    a.dff = dff;
    a.eps = eps;
    a.act = act == CN_ACT_SWISH ? FF_ACT_SWISH : FF_ACT_RELU;
    if (!sc.ok()) return -2;
    return sc.finish(launch_ffn_x3(a, (hipStream_t)stream));
}

// The row-chain form of the split-bf16 engine as one op (fused_x3.hip PRO / TAIL): x += Wo . ctx + bo; x += FFN(LN1 x); then
// LN_next(x) -> xn_out_dev (wt_host null) or its projection Wt . LN_next(x) + bt -> tail_out_dev (split-bf16 rows of tail_n
// elements).  ctx_dev: split-bf16 [M][256] or null (no output projection); weight matrices on the host (fp32, nn.Linear layout),
// vectors on the device.
extern "C" int cn_op_x3_chain(float* x_dev, const void* ctx_dev, const float* wo_host, const float* bo_dev, const float* ln_a_dev,
                              const float* ln_b_dev, const float* w1_host, const float* b1_dev, const float* w2_host,
                              const float* b2_dev, const float* nln_a_dev, const float* nln_b_dev, void* xn_out_dev,
                              const float* wt_host, const float* bt_dev, void* tail_out_dev, int32_t tail_n, int32_t M, int32_t dff,
                              float eps, int32_t mix, void* stream) {
    // everything launch_ffn_x3 would refuse is refused here, before the weights are packed and anything touches the device
    if (!ffn_x3_applies(256, dff)) {
        cn_set_error("cn_op_x3_chain: d_ff=" + std::to_string(dff) + " must be a multiple of 128 in [128, 2048]");
        return -1;
    }
    if (ffn_x3_form("cn_op_x3_chain", ctx_dev != nullptr, wt_host != nullptr, tail_n, mix != 0, FF_ACT_RELU) < 0) return -1;
    if (wt_host && (!nln_a_dev || !nln_b_dev)) {
        cn_set_error("cn_op_x3_chain: a tail projection needs the next LayerNorm (nln_a_dev, nln_b_dev): it projects LN_next(x)");
        return -1;
    }
    if (wt_host && (!bt_dev || !tail_out_dev)) {
        cn_set_error("cn_op_x3_chain: a tail projection needs its bias and its output (bt_dev, tail_out_dev)");
        return -1;
    }
    if (ctx_dev && (!wo_host || !bo_dev)) {
        cn_set_error("cn_op_x3_chain: ctx_dev needs the output projection's weights and bias (wo_host, bo_dev)");
        return -1;
    }
    Scratch sc("cn_op_x3_chain", (hipStream_t)stream);
    FfnX3Args a;
    {
        std::vector<uint16_t> h(ffn_x3_stream_bytes(dff) / 2);
        pack_ffn_x3(w1_host, w2_host, dff, h.data(), mix != 0);
        a.wst = sc.upload(h.data(), h.size() * 2);
        a.mix = mix != 0;
    }
    if (ctx_dev) {
        std::vector<unsigned char> h((size_t)256 * 1024);
        pack_proj_x3(wo_host, 256, h.data());
        a.ctx = ctx_dev;
        a.wo_p = sc.upload(h.data(), h.size());
        a.bo = bo_dev;
    }
    if (wt_host) {
        std::vector<unsigned char> h((size_t)tail_n * 1024);
        pack_proj_x3(wt_host, tail_n, h.data());
        a.tail_p = sc.upload(h.data(), h.size());
        a.tail_b = bt_dev;
        a.tail_out = tail_out_dev;
        a.tail_n = tail_n;
        a.ld_tail = tail_n;
    }
    a.x = x_dev;
    a.ln_a = ln_a_dev;
    a.ln_b = ln_b_dev;
    a.b1 = b1_dev;
    a.b2 = b2_dev;
    a.nln_a = nln_a_dev;
    a.nln_b = nln_b_dev;
    a.xn_out = xn_out_dev;
    a.M = M;
    a.d = 256;
    a.dff = dff;
    a.eps = eps;
    if (!sc.ok()) return -2;
    return sc.finish(launch_ffn_x3(a, (hipStream_t)stream));
}

// Every ChainArgs field from the descriptor.  `who`: the entry's name for messages.  Everything the launcher would refuse is refused
// here, before the weights are packed and anything touches the device.
static int op_chain_desc(const char* who, const cn_chain_desc* d, void* stream) {
    auto refuse = [&](const char* why) {
        cn_set_error((std::string(who) + ": " + why).c_str());
        return -1;
    };
    if (!d) return refuse("null descriptor");
    const int32_t dff = d->dff, tail_n = d->tail_n;
    if (dff < 0 || dff % 128 != 0 || dff > 2048 || tail_n < 0 || tail_n % 256 != 0 || tail_n > 1536)
        return refuse("d_ff must be a multiple of 128 (<= 2048) and the tail width a multiple of 256 (<= 1536)");
    if (!d->x) return refuse("null x");
    if (d->ctx && (!d->wo || !d->bo)) return refuse("ctx needs wo and bo");
    if (dff > 0 && (!d->ln1_a || !d->ln1_b || !d->w1 || !d->b1 || !d->w2 || !d->b2))
        return refuse("d_ff > 0 needs ln1_a, ln1_b, w1, b1, w2 and b2");
    const bool has_next = d->nln_a != nullptr;
    if (has_next && !d->nln_b) return refuse("nln_a needs nln_b");
    if (tail_n > 0 && (!has_next || !d->out || !d->wt || !d->bt)) return refuse("a tail needs nln_a, nln_b, wt, bt and out");
    if (has_next && !d->out && !d->ln_out) return refuse("LNn(x) needs out or ln_out");
    if (d->ln_out && !has_next) return refuse("ln_out needs nln_a and nln_b");
    const int f8 = d->f8 != 0;
    if (f8 && (dff <= 0 || dff % 256 != 0 || d->swish))
        return refuse("the e4m3 feed-forward form (x_mode bit 32) needs d_ff % 256 == 0 and the ReLU activation");
    if (d->rows_dev && d->swish) return refuse("a device-side row count exists for the ReLU forms (the transformer decoder side)");
    if (d->ctx && d->ctx_blocked && d->ldctx != 256) return refuse("a blocked ctx has 256 columns (ldctx == 256)");
    if (d->ctx && !d->ctx_blocked && (d->ldctx < 256 || d->ldctx % 8 != 0))
        return refuse("row-major ctx rows hold 256 columns and are 16-byte aligned (ldctx >= 256, % 8 == 0)");
    // where LNn(x) goes and with which row stride (launch_chain): ln_out, else `out` of a launch without tail
    const bool ln_to_out = has_next && !d->ln_out && tail_n == 0;
    const int32_t ld_ln = d->ln_out ? d->ld_ln : d->ldo;
    if (has_next && (d->ln_out || ln_to_out)) {
        if (d->ln_blocked && ld_ln != 256)
            return refuse("a blocked LNn(x) has 256 columns (ld_ln == 256, or ldo == 256 where out takes it)");
        if (!d->ln_blocked && (ld_ln < 256 || ld_ln % 4 != 0))
            return refuse("row-major LNn(x) rows hold 256 columns and are 8-byte aligned (ld >= 256, % 4 == 0)");
    }
    if (tail_n > 0) {
        if (d->out_blocked && (d->ldo < tail_n || d->ldo % 32 != 0))
            return refuse("a blocked tail output needs ldo % 32 == 0 and ldo >= tail_n");
        if (!d->out_blocked && (d->ldo < tail_n || d->ldo % 8 != 0))
            return refuse("row-major tail rows hold tail_n columns and are 16-byte aligned (ldo >= tail_n, % 8 == 0)");
    }
    if (d->M < 0) return refuse("M < 0");
    ChainWeights w;
    w.wo = d->ctx ? d->wo : nullptr;
    w.bo = d->bo;
    w.ln1_a = d->ln1_a;
    w.ln1_b = d->ln1_b;
    w.w1 = d->w1;
    w.b1 = d->b1;
    w.w2 = d->w2;
    w.b2 = d->b2;
    w.nln_a = d->nln_a;
    w.nln_b = d->nln_b;
    w.wt = d->wt;
    w.bt = d->bt;
    w.dff = dff;
    w.tail_n = tail_n;
    const size_t units = chain_stream_units(d->ctx != nullptr, dff, tail_n, f8);
    std::vector<uint16_t> hs((units + 7) * (CHAIN_UNIT_BYTES / 2));  // (seven spare units: the kernel's dummy refills read them)
    std::vector<float> ht(CHAIN_TAB_FLOATS + 4);  // the table, then the four scale bytes of the e4m3 form
    int hq[4] = {127, 127, 127, 127};
    pack_chain(w, hs.data(), ht.data(), f8 ? hq : nullptr);
    std::memcpy(&ht[CHAIN_TAB_FLOATS], hq, 16);
    Scratch sc(who, (hipStream_t)stream);
    void* ds = sc.upload(hs.data(), hs.size() * 2);
    const float* dt = (const float*)sc.upload(ht.data(), ht.size() * 4);
    if (!sc.ok()) return -2;
    ChainArgs a;
    a.x = d->x;
    a.ctx = d->ctx;
    a.ldctx = d->ldctx;
    a.ctx_blocked = d->ctx_blocked != 0;
    a.wstream = ds;
    a.tab = dt;
    a.out = d->out;
    a.ldo = d->ldo;
    a.ln_out = d->ln_out;
    a.ld_ln = d->ld_ln;
    a.M = d->M;
    a.m_dev = d->rows_dev;
    a.d = 256;
    a.dff = dff;
    a.tail_n = tail_n;
    a.has_next = has_next;
    a.eps = d->eps;
    a.x_in_blocked = d->x_in_blocked != 0;
    a.x_out_blocked = d->x_out_blocked != 0;
    a.store_x = d->store_x != 0;
    a.swish = d->swish != 0;
    a.out_blocked = d->out_blocked != 0;
    a.ln_blocked = d->ln_blocked != 0;
    a.f8 = f8;
    a.f8_q = f8 ? reinterpret_cast<const int*>(dt + CHAIN_TAB_FLOATS) : nullptr;
    int rc = launch_chain(a, (hipStream_t)stream);
    if (const char* rep = cn_exp_env("CASSNAT_CHAIN_REPEAT")) {  // timing runs only: x keeps being updated
        // CASSNAT_CHAIN_STREAMS = n: the repeats go round-robin onto n private streams (how do concurrent launches share
        // the chip?); they race on x, which a timing run does not look at
        const int ns = cn_exp_env("CASSNAT_CHAIN_STREAMS") ? atoi(cn_exp_env("CASSNAT_CHAIN_STREAMS")) : 0;
        std::vector<hipStream_t> ss(ns > 0 ? ns : 0);
        for (auto& q : ss) (void)hipStreamCreateWithFlags(&q, hipStreamNonBlocking);
        (void)hipStreamSynchronize((hipStream_t)stream);
        for (int i = 1; i < atoi(rep) && rc == 0; ++i) rc = launch_chain(a, ns > 0 ? ss[i % ns] : (hipStream_t)stream);
        for (auto& q : ss) {
            (void)hipStreamSynchronize(q);
            (void)hipStreamDestroy(q);
        }
    }
    rc = sc.finish(rc);
    if (cn_exp_env("CASSNAT_CHAIN_STAMPS")) (void)chain_print_stamps();
    return rc;
}

// cn_op_chain / cn_op_chain_rows: the descriptor with the x_mode bits spelled out
static cn_chain_desc chain_desc_of(float* x_dev, const void* ctx_dev, int32_t ldctx, const float* wo_host, const float* bo_host,
                                   const float* ln1_a_host, const float* ln1_b_host, const float* w1_host, const float* b1_host,
                                   const float* w2_host, const float* b2_host, const float* nln_a_host, const float* nln_b_host,
                                   const float* wt_host, const float* bt_host, void* out_dev, int32_t ldo, int32_t M, int32_t dff,
                                   int32_t tail_n, float eps, int32_t x_mode, const int32_t* rows_dev) {
    cn_chain_desc d = {};
    d.x = x_dev;
    d.ctx = ctx_dev;
    d.ldctx = ldctx;
    d.wo = wo_host;
    d.bo = bo_host;
    d.ln1_a = ln1_a_host;
    d.ln1_b = ln1_b_host;
    d.w1 = w1_host;
    d.b1 = b1_host;
    d.w2 = w2_host;
    d.b2 = b2_host;
    d.nln_a = nln_a_host;
    d.nln_b = nln_b_host;
    d.wt = wt_host;
    d.bt = bt_host;
    d.out = out_dev;
    d.ldo = ldo;
    d.M = M;
    d.dff = dff;
    d.tail_n = tail_n;
    d.eps = eps;
    d.x_in_blocked = (x_mode & 1) != 0;
    d.x_out_blocked = (x_mode & 2) != 0;
    d.store_x = (x_mode & 4) == 0;
    d.swish = (x_mode & 8) != 0;
    d.out_blocked = (x_mode & 16) != 0;
    d.f8 = (x_mode & 32) != 0;
    d.ln_blocked = (x_mode & 64) != 0;
    d.rows_dev = rows_dev;
    return d;
}

extern "C" int cn_op_chain(float* x_dev, const void* ctx_dev, int32_t ldctx, const float* wo_host, const float* bo_host,
                           const float* ln1_a_host, const float* ln1_b_host, const float* w1_host, const float* b1_host,
                           const float* w2_host, const float* b2_host, const float* nln_a_host, const float* nln_b_host,
                           const float* wt_host, const float* bt_host, void* out_dev, int32_t ldo, int32_t M, int32_t dff,
                           int32_t tail_n, float eps, int32_t x_mode, void* stream) {
    const cn_chain_desc d = chain_desc_of(x_dev, ctx_dev, ldctx, wo_host, bo_host, ln1_a_host, ln1_b_host, w1_host, b1_host, w2_host,
                                          b2_host, nln_a_host, nln_b_host, wt_host, bt_host, out_dev, ldo, M, dff, tail_n, eps, x_mode,
                                          nullptr);
    return op_chain_desc("cn_op_chain", &d, stream);
}

extern "C" int cn_op_chain_rows(float* x_dev, const void* ctx_dev, int32_t ldctx, const float* wo_host, const float* bo_host,
                                const float* ln1_a_host, const float* ln1_b_host, const float* w1_host, const float* b1_host,
                                const float* w2_host, const float* b2_host, const float* nln_a_host, const float* nln_b_host,
                                const float* wt_host, const float* bt_host, void* out_dev, int32_t ldo, int32_t M, int32_t dff,
                                int32_t tail_n, float eps, int32_t x_mode, const int32_t* rows_dev, void* stream) {
    if (!rows_dev) {
        cn_set_error("cn_op_chain_rows: null row count");
        return -1;
    }
    const cn_chain_desc d = chain_desc_of(x_dev, ctx_dev, ldctx, wo_host, bo_host, ln1_a_host, ln1_b_host, w1_host, b1_host, w2_host,
                                          b2_host, nln_a_host, nln_b_host, wt_host, bt_host, out_dev, ldo, M, dff, tail_n, eps, x_mode,
                                          rows_dev);
    return op_chain_desc("cn_op_chain_rows", &d, stream);
}

extern "C" int cn_op_chain_desc(const cn_chain_desc* d, void* stream) { return op_chain_desc("cn_op_chain_desc", d, stream); }
extern "C" int32_t cn_chain_desc_size(void) { return (int32_t)sizeof(cn_chain_desc); }

// cn_genmax_desc -> GenmaxArgs without the packed operands: the checks of the descriptor itself (cassnat_hip_genmax.h lists them);
// the shape and pointer-combination checks are decide_genmax's, which launch_genmax runs for the engine's calls too.  0, or -1 with
// the error set.  Nothing is sized from V here: genmax_vtw of a V below -127 is negative.
static int genmax_args_of(const char* who, const cn_genmax_desc* d, GenmaxArgs* a) {
    auto refuse = [&](const char* what) {
        cn_set_error(std::string(who) + ": " + what);
        return -1;
    };
    if (!d) return refuse("null descriptor");
    if (d->reserved != 0) return refuse("the reserved word must be 0");
    if (d->precision != CN_PRECISION_BF16 && d->precision != CN_PRECISION_F16 && d->precision != CN_PRECISION_BF16X3)
        return refuse("precision must be the library's 16-bit operand (CN_PRECISION_BF16 or CN_PRECISION_F16) or CN_PRECISION_BF16X3");
    const int prec = cn_own_precision(d->precision, who);
    if (prec < 0) return -1;
    if (!d->h_dev || !d->w_host || !d->b_host) return refuse("null h_dev, w_host or b_host");
    *a = GenmaxArgs();
    a->x3 = prec == CN_PREC_X3;
    a->h = d->h_dev;
    a->arg = d->arg_dev;
    a->maxlp = d->maxlp_dev;
    a->M = d->M;
    a->V = d->V;
    a->d = 256;
    a->m_dev = d->m_dev;
    a->tgt = d->tgt_dev;
    a->tgt_lp = d->tgt_lp_dev;
    a->tgt_U = d->U;
    a->tgt_ld = d->ld;
    return 0;
}

static int op_genmax_desc(const char* who, const cn_genmax_desc* d, void* stream) {
    GenmaxArgs a;
    GenmaxForm f;
    if (genmax_args_of(who, d, &a) != 0 || decide_genmax(a, &f, who, false) != 0) return -1;
    if (f.mt == 0) return 0;
    const size_t waves = a.x3 ? 8 : 4;
    std::vector<uint16_t> hw(waves * f.vtw * 16 * (a.x3 ? 1024 : 512));
    std::vector<float> hb(waves * f.vtw * 32);
    (a.x3 ? pack_genmax_x3 : pack_genmax)(d->w_host, d->b_host, a.V, hw.data(), hb.data());
    Scratch sc(who, (hipStream_t)stream);
    a.wp = sc.upload(hw.data(), hw.size() * 2);
    a.bp = (const float*)sc.upload(hb.data(), hb.size() * 4);
    if (!sc.ok()) return -2;
    int rc = launch_genmax(a, (hipStream_t)stream);
    if (const char* rep = cn_exp_env("CASSNAT_GENMAX_REPEAT"))  // timing runs only
        for (int i = 1, n = atoi(rep); rc == 0 && i < n; ++i) rc = launch_genmax(a, (hipStream_t)stream);
    return sc.finish(rc);
}

extern "C" int cn_op_genmax_desc(const cn_genmax_desc* d, void* stream) { return op_genmax_desc("cn_op_genmax_desc", d, stream); }
extern "C" int32_t cn_genmax_desc_size(void) { return (int32_t)sizeof(cn_genmax_desc); }

static_assert(CN_GENMAX_KIND_ARGMAX_LSE == GENMAX_ARGMAX_LSE && CN_GENMAX_KIND_ARGMAX == GENMAX_ARGMAX && CN_GENMAX_KIND_GATHER == GENMAX_GATHER,
              "the public output kinds are the kernel's");

extern "C" int32_t cn_genmax_form_launch(const cn_genmax_desc* d, int32_t* lds_bytes, int32_t* grid) {
    GenmaxArgs a;
    GenmaxForm f;
    if (genmax_args_of("cn_genmax_form", d, &a) != 0 || decide_genmax(a, &f, "cn_genmax_form", false) != 0) return -1;
    if (lds_bytes) *lds_bytes = f.lds;
    if (grid) *grid = f.grid;
    return (f.x3 ? CN_GENMAX_KERNEL_SPLIT : CN_GENMAX_KERNEL_16) | f.mt << 4 | f.kind << 8 | f.vtw << 12;
}
extern "C" int32_t cn_genmax_form(const cn_genmax_desc* d) { return cn_genmax_form_launch(d, nullptr, nullptr); }

extern "C" int cn_genmax_pack(int32_t precision, const float* w_host, const float* b_host, int32_t V, void* w_out, int64_t w_bytes,
                              float* b_out, int64_t b_floats) {
    static const int32_t one = 0;  // (a stand-in for the descriptor's device pointers: the checks follow none)
    cn_genmax_desc d = {};
    d.precision = precision;
    d.h_dev = &one;
    d.w_host = w_host;
    d.b_host = b_host;
    d.M = 0;
    d.V = V;
    d.arg_dev = const_cast<int32_t*>(&one);
    GenmaxArgs a;
    GenmaxForm f;
    if (genmax_args_of("cn_genmax_pack", &d, &a) != 0 || decide_genmax(a, &f, "cn_genmax_pack", false) != 0) return -1;
    const int64_t waves = a.x3 ? 8 : 4, wb = waves * f.vtw * (a.x3 ? 32768 : 16384), bf = waves * f.vtw * 32;
    if (!w_out || !b_out || w_bytes != wb || b_floats != bf) {
        cn_set_error("cn_genmax_pack: V=" + std::to_string(V) + " packs into exactly " + std::to_string(wb) + " bytes of weights and " +
                     std::to_string(bf) + " biases (non-null buffers of that size)");
        return -1;
    }
    (a.x3 ? pack_genmax_x3 : pack_genmax)(w_host, b_host, V, static_cast<uint16_t*>(w_out), b_out);
    return 0;
}

#ifdef CN_OP16_F16
static const int32_t kOwn16 = CN_PRECISION_F16;
#else
static const int32_t kOwn16 = CN_PRECISION_BF16;
#endif

static cn_genmax_desc genmax_desc_of(int32_t precision, const void* h_dev, const float* w_host, const float* b_host, int32_t M, int32_t V,
                                     int32_t* arg_dev, float* maxlp_dev, const int32_t* tgt_dev, int32_t U, int32_t ld, float* tgt_lp_dev) {
    cn_genmax_desc d = {};
    d.precision = precision;
    d.h_dev = h_dev;
    d.w_host = w_host;
    d.b_host = b_host;
    d.M = M;
    d.V = V;
    d.arg_dev = arg_dev;
    d.maxlp_dev = maxlp_dev;
    d.tgt_dev = tgt_dev;
    d.U = U;
    d.ld = ld;
    d.tgt_lp_dev = tgt_lp_dev;
    return d;
}

extern "C" int cn_op_genmax(const void* h_dev, const float* w_host, const float* b_host, int32_t M, int32_t V,
                            int32_t* arg_dev, float* maxlp_dev, void* stream) {
    const cn_genmax_desc d = genmax_desc_of(kOwn16, h_dev, w_host, b_host, M, V, arg_dev, maxlp_dev, nullptr, 0, 0, nullptr);
    return op_genmax_desc("cn_op_genmax", &d, stream);
}

extern "C" int cn_op_genmax_gather(const void* h_dev, const float* w_host, const float* b_host, int32_t B, int32_t U, int32_t V,
                                   const int32_t* tgt_dev, int32_t ld, float* tgt_lp_dev, void* stream) {
    if (B < 0 || U < 1 || (int64_t)B * U > INT32_MAX) {
        cn_set_error("cn_op_genmax_gather: B must not be negative, U at least 1 and B x U an int32");
        return -1;
    }
    const cn_genmax_desc d = genmax_desc_of(kOwn16, h_dev, w_host, b_host, B * U, V, nullptr, nullptr, tgt_dev, U, ld, tgt_lp_dev);
    return op_genmax_desc("cn_op_genmax_gather", &d, stream);
}

// the split-bf16 form (CN_PRECISION_BF16X3): h_host fp32 [M][256] is split into hi + lo halves and uploaded by the call;
// tgt_dev == NULL: arg-max (+ maxlp when maxlp_dev), else the target gather with M = rows, U per sequence, ld the target stride
extern "C" int cn_op_genmax_x3(const float* h_host, const float* w_host, const float* b_host, int32_t M, int32_t V, int32_t* arg_dev,
                               float* maxlp_dev, const int32_t* tgt_dev, int32_t U, int32_t ld, float* tgt_lp_dev, void* stream) {
    // the descriptor's checks first, with the host rows standing in for the device's: nothing is split or uploaded for a refused call
    cn_genmax_desc d = genmax_desc_of(CN_PRECISION_BF16X3, h_host, w_host, b_host, M, V, arg_dev, maxlp_dev, tgt_dev, U, ld, tgt_lp_dev);
    GenmaxArgs a;
    GenmaxForm f;
    if (genmax_args_of("cn_op_genmax_x3", &d, &a) != 0 || decide_genmax(a, &f, "cn_op_genmax_x3", false) != 0) return -1;
    if (f.mt == 0) return 0;
    const std::vector<unsigned char> hx = split_rows256(h_host, M);
    Scratch sc("cn_op_genmax_x3", (hipStream_t)stream);
    d.h_dev = sc.upload(hx.data(), hx.size());
    if (!sc.ok()) return -2;
    return sc.finish(op_genmax_desc("cn_op_genmax_x3", &d, stream));
}

// d_model-deep projection of the split-bf16 engine (proj_x3.hip): a_host fp32 [M][256] and w_host fp32 [N][256] are split into
// hi + lo halves, packed and uploaded by the call; bias_host [N].  split_out == 0: c_dev fp32 [M][N] = (resid_dev ? resid +
// resid_scale * : ) (A . W^T + bias), resid_dev fp32 [M][N] may alias c_dev;  split_out == 1: c_dev receives split-bf16 rows
// (M * N * 4 bytes: per 32 columns 64 bytes of hi halves, then 64 bytes of lo halves)
extern "C" int cn_op_proj_x3(const float* a_host, const float* w_host, const float* bias_host, const float* resid_dev,
                             float resid_scale, void* c_dev, int32_t M, int32_t N, int32_t split_out, void* stream) {
    if (!proj_x3_applies(N, 256) || M < 1) {
        cn_set_error("cn_op_proj_x3: N must be a multiple of 32, at most 1024");
        return -1;
    }
    const std::vector<unsigned char> hx = split_rows256(a_host, M);
    Scratch sc("cn_op_proj_x3", (hipStream_t)stream);
    cn_proj_x3_desc d = {};
    d.a_dev = sc.upload(hx.data(), hx.size());
    if (!sc.ok()) return -2;
    d.w_host = w_host;
    d.bias_host = bias_host;
    d.c_dev = c_dev;
    d.resid_dev = resid_dev;
    d.lda = 256;
    d.ldc = d.ldr = N;
    d.M = M;
    d.N = N;
    d.split_out = split_out;
    d.resid_scale = resid_scale;
    return cn_op_proj_x3_desc(&d, stream);
}

// The same projection through a descriptor that reaches every field of ProjX3Args: A is on the device already (split-bf16 rows of
// lda elements), every stride is the caller's.  Everything launch_proj_x3 would refuse is refused here, before the weights are
// packed and anything touches the device.
extern "C" int cn_op_proj_x3_desc(const cn_proj_x3_desc* d, void* stream) {
    auto refuse = [](const std::string& why) {
        cn_set_error("cn_op_proj_x3_desc: " + why);
        return -1;
    };
    if (!d) return refuse("null descriptor");
    if (!d->a_dev || !d->w_host || !d->bias_host || !d->c_dev) return refuse("null a_dev, w_host, bias_host or c_dev");
    if (d->reserved != 0) return refuse("the reserved word must be 0");
    if (d->M < 0) return refuse("M=" + std::to_string(d->M) + " is negative");
    if (d->split_out != 0 && d->split_out != 1) return refuse("split_out must be 0 or 1");
    ProjX3Args a;
    a.A = d->a_dev;
    a.lda = d->lda;
    a.C = d->c_dev;
    a.ldc = d->ldc;
    a.c_f32 = d->split_out ? 0 : 1;
    a.resid = d->resid_dev;
    a.ldr = d->ldr;
    a.resid_scale = d->resid_scale;
    a.M = d->M;
    a.N = d->N;
    if (const char* why = proj_x3_refusal(a, false))
        return refuse(std::string(why) + " (lda=" + std::to_string(d->lda) + " ldc=" + std::to_string(d->ldc) + " ldr=" +
                      std::to_string(d->ldr) + " M=" + std::to_string(d->M) + " N=" + std::to_string(d->N) + ")");
    if (d->M == 0) return 0;
    std::vector<unsigned char> hw((size_t)d->N * 1024);
    pack_proj_x3(d->w_host, d->N, hw.data());
    Scratch sc("cn_op_proj_x3_desc", (hipStream_t)stream);
    a.wp = sc.upload(hw.data(), hw.size());
    a.bias = (const float*)sc.upload(d->bias_host, (size_t)d->N * 4);
    if (!sc.ok()) return -2;
    return sc.finish(launch_proj_x3(a, (hipStream_t)stream));
}
extern "C" int32_t cn_proj_x3_desc_size(void) { return (int32_t)sizeof(cn_proj_x3_desc); }

// what launch_proj_x3 launches for (M, N): *mt = 32-row tiles per workgroup (1 or 2), *chunks = column chunks (gridDim.y)
extern "C" int cn_proj_x3_form(int32_t M, int32_t N, int32_t split_out, int32_t* mt, int32_t* chunks) {
    if (!mt || !chunks || M < 1 || !proj_x3_applies(N, 256) || (split_out != 0 && split_out != 1)) {
        cn_set_error("cn_proj_x3_form: needs M >= 1, N a multiple of 32 in [32, 1024], split_out 0 or 1 and both result pointers");
        return -1;
    }
    int mt_, chunks_;
    proj_x3_form(M, N, &mt_, &chunks_);
    *mt = mt_;
    *chunks = chunks_;
    return 0;
}

// the instantiation launch_ffn_x3 picks: *form = a sum of CN_FFN_X3_PRO / TAIL / MIX / SWISH; tail_n == 0: no tail
extern "C" int cn_ffn_x3_form(int32_t has_ctx, int32_t tail_n, int32_t mix, int32_t act, int32_t* form) {
    if (!form) {
        cn_set_error("cn_ffn_x3_form: null result pointer");
        return -1;
    }
    if (act != CN_ACT_RELU && act != CN_ACT_SWISH) {
        cn_set_error("cn_ffn_x3_form: unknown activation");
        return -1;
    }
    const int f = ffn_x3_form("cn_ffn_x3_form", has_ctx != 0, tail_n != 0, tail_n, mix != 0, act == CN_ACT_SWISH ? FF_ACT_SWISH : FF_ACT_RELU);
    if (f < 0) return -1;
    *form = f;
    return 0;
}
static_assert(CN_FFN_X3_PRO == FFN_X3_PRO && CN_FFN_X3_TAIL == FFN_X3_TAIL && CN_FFN_X3_MIX == FFN_X3_MIX && CN_FFN_X3_SWISH == FFN_X3_SWISH,
              "cassnat_hip.h and kernels.h name the same bits");
