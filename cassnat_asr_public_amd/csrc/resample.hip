// Sample-rate conversion and channel pick in front of the fbank kernel: what Kaldi's compute-fbank-feats does with a file whose
// rate differs from --sample-frequency (--allow-downsample / --allow-upsample -> ResampleWaveform) or that holds several channels
// (--channel).  Algorithm = kaldi-asr/kaldi src/feat/resample.cc, LinearResample as ResampleWaveform configures it (num_zeros 6,
// cutoff 0.99 * 0.5 * min(rates)): a windowed-sinc filter, one weight row per output phase (out_rate / gcd phases), the number of
// outputs as GetNumOutputSamples gives it with flush = true.  Parity is pinned to tests/resample_model.py, the float64
// restatement (the reference tree never opens a sound file).
//
// One output per lane, RS_RUN consecutive outputs of one utterance per workgroup.  The workgroup stages the input span its outputs
// need - about RS_RUN * in_rate / out_rate + taps samples, the chosen channel of the interleaved int16 picked on the load - into LDS
// as float; each lane then sums its phase's taps in ascending order (float32, fmaf).  The weights stay in global memory, tap-major
// ([tap][phase]: consecutive lanes are consecutive phases), at most 256 KiB and shared by every workgroup.  HBM-bound:
// 2 * channels * in_rate / out_rate bytes in and 4 bytes out per output sample; no matrix cores.
#include <cmath>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "kernels.h"

constexpr int RS_RUN = 256;             // outputs (= lanes) per workgroup
constexpr int RS_TILE = 4096;           // floats of LDS per workgroup: 16 KiB, eight workgroups of four waves per CU keep their 32 waves
constexpr int RS_MAX_WEIGHTS = 65536;   // phases x taps

struct ResampleParams {
    const unsigned char* staged;  // the utterances' interleaved int16 as the WAV data chunks hold them, utterance r at byte off[r]
    long long staged_bytes;
    const int* off;               // [utts] byte offsets
    const int* samples;           // [utts] samples per channel
    const int* channels;          // [utts]
    const int* channel;           // [utts] the channel that is read
    const int* rows;              // [n_rows] utterance indices, or null: 0 .. n_rows - 1
    float* out;                   // utterance r's outputs at out + out_off[r]
    const int* out_off;           // [utts] float offsets
    const int* first;             // [out_unit] first input index of phase p (relative to u * in_unit)
    const int* taps;              // [out_unit]
    const float* weights;         // [max_taps][out_unit]
    int utts, in_unit, out_unit;
};

__global__ __launch_bounds__(RS_RUN) void wave_resample_kernel(ResampleParams p) {
    __shared__ float x[RS_TILE];
    const int r = p.rows ? p.rows[blockIdx.y] : (int)blockIdx.y;
    if (r < 0 || r >= p.utts) return;
    const long long o0 = p.off[r];
    const int C = p.channels[r], c = p.channel[r];
    long long ns = p.samples[r];
    // reads stay inside [0, staged_bytes): an utterance that reaches outside is cut to the sample frames that lie inside
    if (C < 1 || c < 0 || c >= C || ns < 0 || o0 < 0 || o0 >= p.staged_bytes) ns = 0;
    else if (o0 + 2LL * C * ns > p.staged_bytes) ns = (p.staged_bytes - o0) / (2LL * C);
    const long long count = (ns * p.out_unit + p.in_unit - 1) / p.in_unit;  // GetNumOutputSamples, flush = true
    const long long k0 = (long long)blockIdx.x * RS_RUN;
    if (k0 >= count) return;  // (uniform over the workgroup)
    const long long k1 = (k0 + RS_RUN <= count ? k0 + RS_RUN : count) - 1;  // the run's last output
    // first input index of an output rises with the output (checked on the host when the table is built), so does the last:
    // the run needs [start of k0, end of k1]
    const int p0 = (int)(k0 % p.out_unit), p1 = (int)(k1 % p.out_unit);
    const long long start = (k0 / p.out_unit) * p.in_unit + p.first[p0];
    const long long stop = (k1 / p.out_unit) * p.in_unit + p.first[p1] + p.taps[p1];  // (one past the last)
    const int span = (int)(stop - start);  // <= RS_TILE: the host refuses a rate pair whose longest span is not
    const short* src = reinterpret_cast<const short*>(p.staged + o0);
    for (int i = threadIdx.x; i < span; i += RS_RUN) {
        const long long g = start + i;
        x[i] = (g >= 0 && g < ns) ? (float)src[g * C + c] : 0.f;
    }
    __syncthreads();
    const long long k = k0 + threadIdx.x;
    if (k > k1) return;
    const int ph = (int)(k % p.out_unit);
    const float* xs = x + (int)((k / p.out_unit) * p.in_unit + p.first[ph] - start);
    const float* w = p.weights + ph;
    const int n = p.taps[ph];
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc = fmaf(w[(long long)j * p.out_unit], xs[j], acc);
    p.out[(long long)p.out_off[r] + k] = acc;
}

// ---- host: the weight table of a rate pair, built in double and rounded to float32 once ---------------------------
namespace {
struct ResampleTable {
    int in_rate = 0, out_rate = 0, in_unit = 0, out_unit = 0, max_taps = 0, max_span = 0;
    std::vector<int> first, taps;
    std::vector<float> weights;  // [max_taps][out_unit]
};

struct ResampleDev {
    int device = -1, in_rate = 0, out_rate = 0, in_unit = 0, out_unit = 0;
    int *first = nullptr, *taps = nullptr;
    float* weights = nullptr;
};
std::vector<ResampleDev> g_rs;  // (a handful of rate pairs per device: a list, kept for the life of the process)
std::mutex g_rs_lock;           // (the decode pipelines' host threads all come through resample_dev)
}  // namespace

static int resample_table_host(int in_rate, int out_rate, ResampleTable* t) {
    if (in_rate <= 0 || out_rate <= 0) {
        cn_set_error("resample: the rates must be positive");
        return -1;
    }
    const int g = std::gcd(in_rate, out_rate);
    t->in_rate = in_rate;
    t->out_rate = out_rate;
    t->in_unit = in_rate / g;
    t->out_unit = out_rate / g;
    if (in_rate == out_rate) {  // nothing is resampled (Kaldi does not call the resampler): the value itself
        t->max_taps = 1;
        t->first.assign(1, 0);
        t->taps.assign(1, 1);
        t->weights.assign(1, 1.0f);
        t->max_span = RS_RUN;
        return 0;
    }
    const double fi = in_rate, fo = out_rate, num_zeros = 6.0;
    const double cutoff = 0.99 * 0.5 * (in_rate < out_rate ? in_rate : out_rate);
    const double window_width = num_zeros / (2.0 * cutoff);
    // every phase has at most 2 * window_width * fi + 1 taps: refuse before anything of that size is built
    if ((2.0 * window_width * fi + 2.0) * t->out_unit > 4.0 * RS_MAX_WEIGHTS) {
        cn_set_error("resample: " + std::to_string(in_rate) + " -> " + std::to_string(out_rate) + " Hz needs a table of more than " +
                     std::to_string(RS_MAX_WEIGHTS) + " weights");
        return -1;
    }
    t->first.resize(t->out_unit);
    t->taps.resize(t->out_unit);
    std::vector<std::vector<double>> w(t->out_unit);
    t->max_taps = 0;
    for (int i = 0; i < t->out_unit; ++i) {
        const double tt = i / fo;
        const int first = (int)std::ceil((tt - window_width) * fi), last = (int)std::floor((tt + window_width) * fi);
        t->first[i] = first;
        t->taps[i] = last - first + 1;
        if (t->taps[i] > t->max_taps) t->max_taps = t->taps[i];
        for (int j = first; j <= last; ++j) {
            const double d = j / fi - tt;
            const double win = std::fabs(d) < window_width ? 0.5 * (1.0 + std::cos(2.0 * M_PI * cutoff / num_zeros * d)) : 0.0;
            const double filt = d != 0.0 ? std::sin(2.0 * M_PI * cutoff * d) / (M_PI * d) : 2.0 * cutoff;
            w[i].push_back(filt * win / fi);
        }
    }
    if ((long long)t->max_taps * t->out_unit > RS_MAX_WEIGHTS) {
        cn_set_error("resample: " + std::to_string(in_rate) + " -> " + std::to_string(out_rate) + " Hz needs a table of " +
                     std::to_string((long long)t->max_taps * t->out_unit) + " weights, more than " + std::to_string(RS_MAX_WEIGHTS));
        return -1;
    }
    t->weights.assign((size_t)t->max_taps * t->out_unit, 0.f);
    for (int i = 0; i < t->out_unit; ++i)
        for (int j = 0; j < t->taps[i]; ++j) t->weights[(size_t)j * t->out_unit + i] = (float)w[i][j];
    // the kernel takes a run's span from its first and its last output: first and end index must not fall from one output to the next
    // (phase out_unit - 1 is followed by phase 0 one in_unit later)
    for (int i = 0; i < t->out_unit; ++i) {
        const int n = (i + 1) % t->out_unit, wrap = i + 1 == t->out_unit ? t->in_unit : 0;
        if (t->first[n] + wrap < t->first[i] || t->first[n] + t->taps[n] + wrap < t->first[i] + t->taps[i] || t->taps[i] < 1) {
            cn_set_error("resample: the table of " + std::to_string(in_rate) + " -> " + std::to_string(out_rate) + " Hz is not monotone");
            return -1;
        }
    }
    // the longest input span of RS_RUN consecutive outputs, over every phase a run can start at
    t->max_span = 0;
    for (int p0 = 0; p0 < t->out_unit; ++p0) {
        const long long k1 = (long long)p0 + RS_RUN - 1;
        const int p1 = (int)(k1 % t->out_unit);
        const long long span = (k1 / t->out_unit) * t->in_unit + t->first[p1] + t->taps[p1] - t->first[p0];
        if (span > RS_TILE) {
            cn_set_error("resample: " + std::to_string(in_rate) + " -> " + std::to_string(out_rate) + " Hz: " + std::to_string(RS_RUN) +
                         " outputs need " + std::to_string(span) + " input samples, the kernel's LDS tile holds " + std::to_string(RS_TILE));
            return -1;
        }
        if (span > t->max_span) t->max_span = (int)span;
    }
    return 0;
}

long long resample_num_samples(int in_rate, int out_rate, long long in_samples) {
    if (in_rate <= 0 || out_rate <= 0 || in_samples <= 0) return 0;
    const long long g = std::gcd(in_rate, out_rate), tick = in_rate / g * out_rate;
    const long long L = in_samples * (tick / in_rate), tpo = tick / out_rate;
    long long last = L / tpo;
    if (last * tpo == L) --last;
    return last + 1;
}

int resample_table(int in_rate, int out_rate, int* in_unit, int* out_unit, int* max_taps, int* first, int* taps, float* weights,
                   long long capacity) {
    ResampleTable t;
    CN_TRY(resample_table_host(in_rate, out_rate, &t));
    *in_unit = t.in_unit;
    *out_unit = t.out_unit;
    *max_taps = t.max_taps;
    if (!first && !taps && !weights) return 0;  // (the sizes alone)
    if (!first || !taps || !weights || capacity < (long long)t.weights.size()) {
        cn_set_error("cn_resample_table: the arrays hold " + std::to_string(capacity) + " weights, the table has " +
                     std::to_string(t.weights.size()));
        return -1;
    }
    std::copy(t.first.begin(), t.first.end(), first);
    std::copy(t.taps.begin(), t.taps.end(), taps);
    std::copy(t.weights.begin(), t.weights.end(), weights);
    return 0;
}

static int resample_dev(int in_rate, int out_rate, ResampleDev* out) {
    int dev = 0;
    CN_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> guard(g_rs_lock);
    for (const ResampleDev& d : g_rs)
        if (d.device == dev && d.in_rate == in_rate && d.out_rate == out_rate) {
            *out = d;
            return 0;
        }
    ResampleTable t;
    CN_TRY(resample_table_host(in_rate, out_rate, &t));
    ResampleDev d;
    d.device = dev;
    d.in_rate = in_rate;
    d.out_rate = out_rate;
    d.in_unit = t.in_unit;
    d.out_unit = t.out_unit;
    CN_HIP_CHECK(hipMalloc((void**)&d.first, t.first.size() * 4));
    CN_HIP_CHECK(hipMalloc((void**)&d.taps, t.taps.size() * 4));
    CN_HIP_CHECK(hipMalloc((void**)&d.weights, t.weights.size() * 4));
    CN_HIP_CHECK(hipMemcpy(d.first, t.first.data(), t.first.size() * 4, hipMemcpyHostToDevice));
    CN_HIP_CHECK(hipMemcpy(d.taps, t.taps.data(), t.taps.size() * 4, hipMemcpyHostToDevice));
    CN_HIP_CHECK(hipMemcpy(d.weights, t.weights.data(), t.weights.size() * 4, hipMemcpyHostToDevice));
    g_rs.push_back(d);
    *out = d;
    return 0;
}

int launch_wave_resample(int in_rate, int out_rate, const unsigned char* staged, long long staged_bytes, const int* off, const int* samples,
                         const int* channels, const int* channel, int utts, const int* rows, int n_rows, long long max_out, float* out,
                         const int* out_off, hipStream_t s) {
    if (n_rows > 65535) {
        cn_set_error("wave_resample: more than 65535 utterances in one call");
        return -1;
    }
    if (max_out > (long long)RS_RUN * 0x7fffffff) {
        cn_set_error("wave_resample: max_out is out of range");
        return -1;
    }
    ResampleDev d;
    CN_TRY(resample_dev(in_rate, out_rate, &d));
    ResampleParams p = {};
    p.staged = staged;
    p.staged_bytes = staged_bytes;
    p.off = off;
    p.samples = samples;
    p.channels = channels;
    p.channel = channel;
    p.rows = rows;
    p.out = out;
    p.out_off = out_off;
    p.first = d.first;
    p.taps = d.taps;
    p.weights = d.weights;
    p.utts = utts;
    p.in_unit = d.in_unit;
    p.out_unit = d.out_unit;
    hipLaunchKernelGGL(wave_resample_kernel, dim3((unsigned)((max_out + RS_RUN - 1) / RS_RUN), n_rows), dim3(RS_RUN), 0, s, p);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}
