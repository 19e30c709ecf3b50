// Stand-alone host check of the energy VAD: the serial twins the library's host entries run (csrc/vad_frames.h: vf_frame_energy_host,
// vf_decide_host - the arithmetic functions the kernels are built from) on the CPU against a naive restatement, every array a heap
// block of exactly the size the functions were told, so that a sanitizer sees any read or write past a span: the staged bytes end
// where staged_bytes says (rows that reach outside are cut to whole sample frames), the outputs hold the frames that exist and a
// sentinel on either side, a recording's decisions end with its last frame.
// Random rows and the extreme ones (a constant frame, all -32768, alternating 32767 / -32768), every channel count, frame lengths
// 1 .. 2048, rows at unaligned even offsets, offsets that are odd, negative or outside; decisions over random quarters with every
// context 0 .. 64 on recordings shorter and longer than the window, one of them empty.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/vad_check.cpp -o vad_check
// Exit status 0 when every check held.
#include <cmath>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "vad_frames.h"

namespace {

int failures = 0;
std::mt19937 rng(12345);

void fail(const char* what, int a, int b) {
    std::printf("FAIL %s (%d, %d)\n", what, a, b);
    ++failures;
}

int pick(int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); }

struct Row {
    std::vector<int16_t> x;  // interleaved
    int lead;                // bytes behind a multiple of 16
    int claim;               // sample frames the caller claims (may exceed what is staged)
};

void energy_case(int N, int shift, int channels, int channel, int remove_dc, std::vector<Row> rows, long long cut, int max_frames) {
    std::vector<int32_t> off, samples, out_off;
    long long at = 0;
    for (auto& r : rows) {
        at = (at + 15) / 16 * 16 + r.lead;
        off.push_back((int32_t)at);
        samples.push_back(r.claim);
        at += (long long)r.x.size() * 2;
    }
    const long long staged_bytes = at - cut;  // (the block ends here: a read behind it is a heap overflow)
    std::unique_ptr<uint8_t[]> staged(new uint8_t[staged_bytes > 0 ? staged_bytes : 1]);
    for (long long i = 0; i < staged_bytes; ++i) staged[i] = (uint8_t)pick(0, 255);
    for (size_t r = 0; r < rows.size(); ++r) {
        const long long n = (long long)rows[r].x.size() * 2, room = staged_bytes - off[r];
        if (room > 0 && n > 0) memcpy(staged.get() + off[r], rows[r].x.data(), (size_t)(n < room ? n : room));
    }
    // the naive restatement: which frames exist, and their values
    std::vector<long long> want_num;
    std::vector<int> frames;
    int total = 1;
    for (size_t r = 0; r < rows.size(); ++r) {
        long long n = 0;
        if (off[r] >= 0 && off[r] % 2 == 0 && samples[r] > 0 && off[r] < staged_bytes) {
            n = (staged_bytes - off[r]) / (2 * channels);
            if (samples[r] < n) n = samples[r];
        }
        int T = n >= N ? (int)(1 + (n - N) / shift) : 0;
        if (T > max_frames) T = max_frames;
        frames.push_back(T);
        out_off.push_back(total);
        for (int t = 0; t < T; ++t) {
            long long S1 = 0, S2 = 0;
            for (int i = 0; i < N; ++i) {
                int16_t v16;  // (from the staged bytes: a row that claims more than it holds reads on into what follows, inside the buffer)
                memcpy(&v16, staged.get() + off[r] + 2 * (((long long)t * shift + i) * channels + channel), 2);
                const long long v = v16;
                S1 += v, S2 += v * v;
            }
            want_num.push_back(remove_dc ? N * S2 - S1 * S1 : S2);
        }
        total += T + 1;  // (a sentinel between the rows)
    }
    std::unique_ptr<int64_t[]> num(new int64_t[total]);
    std::unique_ptr<double[]> e(new double[total]);
    for (int i = 0; i < total; ++i) num[i] = -7, e[i] = -7.5;
    vf_frame_energy_host(staged.get(), staged_bytes, off.data(), samples.data(), out_off.data(), (int)rows.size(), N, shift, channels, channel,
                         remove_dc, max_frames, num.get(), e.get());
    size_t k = 0;
    for (size_t r = 0; r < rows.size(); ++r) {
        if (num[out_off[r] - 1] != -7 || e[out_off[r] - 1] != -7.5) fail("a sentinel in front of a row was written", N, (int)r);
        for (int t = 0; t < frames[r]; ++t, ++k) {
            const long long m = want_num[k];
            if (num[out_off[r] + t] != m || m < 0 || m >= (1LL << 52) + (remove_dc ? 0 : 1)) fail("num", N, t);
            const double E = remove_dc ? (double)m / N : (double)m, want = std::log(E < 0x1p-23 ? 0x1p-23 : E);
            if (!(std::fabs(e[out_off[r] + t] - want) <= 4 * 0x1p-52 * std::fmax(1.0, std::fabs(want)))) fail("e", N, t);
        }
    }
    if (num[total - 1] != -7 || e[total - 1] != -7.5) fail("the sentinel behind the last row was written", N, 0);
}

std::vector<int16_t> noise(int n, int channels) {
    std::vector<int16_t> x((size_t)n * channels);
    for (auto& v : x) v = (int16_t)pick(-32768, 32767);
    return x;
}

void energy_checks() {
    const int leads[4] = {0, 2, 6, 14};
    for (int it = 0; it < 60; ++it) {
        const int N = it < 4 ? (it % 2 ? 2048 : 1) : pick(1, 2048), shift = pick(1, it % 3 ? 700 : 3), channels = pick(1, 8), channel = pick(0, channels - 1);
        std::vector<Row> rows;
        for (int r = 0, R = pick(1, 6); r < R; ++r) {
            const int n = pick(0, 3) ? N + pick(-1, 5 * shift) : pick(0, N);
            const int have = n < 0 ? 0 : n;
            rows.push_back({noise(have, channels), leads[pick(0, 3)], have + (pick(0, 4) ? 0 : pick(1, 1000))});  // (some rows claim more)
        }
        const long long last = (long long)rows.back().x.size() * 2;
        const long long cut = pick(0, 2) ? 0 : pick(0, (int)(last < 4000 ? last : 4000));  // (inside the last row, inside a sample frame)
        energy_case(N, shift, channels, channel, it & 1, rows, cut, pick(0, 3) ? 1 << 20 : pick(1, 4));
    }
    for (int N : {1, 2, 400, 2048})
        for (int remove_dc = 0; remove_dc < 2; ++remove_dc) {
            std::vector<int16_t> lo(N, -32768), c(N, 1234), alt(N);
            for (int i = 0; i < N; ++i) alt[i] = i % 2 ? -32768 : 32767;
            energy_case(N, 1, 1, 0, remove_dc, {{lo, 0, N}, {c, 2, N}, {alt, 14, N}}, 0, 4);
        }
    // offsets that are odd, negative or outside give no frame and are never dereferenced
    {
        std::vector<int16_t> x = noise(64, 1);
        int32_t off[3] = {-16, 1, 1 << 20}, samples[3] = {8, 8, 8}, out_off[3] = {0, 0, 0};
        int64_t num[1] = {-7};
        double e[1] = {-7.5};
        vf_frame_energy_host(reinterpret_cast<const uint8_t*>(x.data()), 128, off, samples, out_off, 3, 4, 2, 1, 0, 1, 8, num, e);
        if (num[0] != -7 || e[0] != -7.5) fail("a row outside the buffer was written", 0, 0);
    }
    if (vf_block_frames(400, 160, 1) != 64 || vf_block_frames(400, 400, 8) != 10 || vf_block_frames(2048, 1 << 30, 8) != 1) fail("vf_block_frames", 0, 0);
    for (int it = 0; it < 2000; ++it) {  // the LDS a launch asks for holds the block's span behind any head, and fits
        const int N = pick(1, 2048), shift = pick(1, 5000), channels = pick(1, 8), F = vf_block_frames(N, shift, channels);
        const long long span = ((long long)(F - 1) * shift + N) * channels * 2;
        if (F < 1 || F > VF_BLOCK_FRAMES || vf_block_bytes(F, N, shift, channels) < span + 14 || vf_block_bytes(F, N, shift, channels) > VF_LDS_BYTES)
            fail("vf_block_bytes", N, shift);
    }
}

void decide_checks() {
    for (int it = 0; it < 200; ++it) {
        const int recs = pick(1, 4), context = it < 65 ? it : pick(0, 64);
        const double proportion = (const double[]){0.0, 0.12, 0.5, 0.6, 1.0}[pick(0, 4)], scale = pick(0, 1) ? 0.5 : 0.0, thr0 = pick(0, 40) / 4.0;
        std::vector<int32_t> off, len;
        int total = 0;
        for (int i = 0; i < recs; ++i) {
            off.push_back(total);
            len.push_back(pick(0, 3) ? pick(1, 200) : 0);
            total += len.back();
        }
        std::unique_ptr<double[]> e(new double[total > 0 ? total : 1]);
        std::unique_ptr<uint8_t[]> dec(new uint8_t[total > 0 ? total : 1]);
        std::unique_ptr<double[]> thr(new double[recs]);
        for (int i = 0; i < total; ++i) e[i] = pick(0, 80) / 4.0, dec[i] = 9;
        vf_decide_host(e.get(), off.data(), len.data(), recs, thr0, scale, context, proportion, thr.get(), dec.get());
        for (int i = 0; i < recs; ++i) {
            const int T = len[i];
            double sum = 0;
            for (int t = 0; t < T; ++t) sum += e[off[i] + t];  // (quarters: exact in any order)
            const double want = (scale == 0.0 || T == 0) ? thr0 : thr0 + scale * (sum / T);
            if (thr[i] != want) fail("thr", i, T);
            for (int t = 0; t < T; ++t) {
                int n = 0, d = 0;
                for (int k = t - context; k <= t + context; ++k)
                    if (k >= 0 && k < T) ++d, n += e[off[i] + k] > want;
                if (dec[off[i] + t] != (uint8_t)((double)n >= (double)d * proportion)) fail("dec", i, t);
            }
        }
    }
    if (vf_check_decide(&failures, &failures, &failures, &failures, &failures, 1, 65) == nullptr || vf_check_decide(&failures, &failures, &failures, &failures, &failures, 0, 0) == nullptr ||
        vf_check_energy(&failures, &failures, &failures, &failures, &failures, &failures, 1, 2049, 1, 1, 0, 1) == nullptr ||
        vf_check_energy(&failures, &failures, &failures, &failures, &failures, &failures, 1, 400, 160, 8, 8, 1) == nullptr ||
        vf_check_energy(&failures, &failures, &failures, &failures, &failures, &failures, 1, 400, 160, 8, 7, 1) != nullptr)
        fail("the refusals", 0, 0);
}

}  // namespace

int main() {
    energy_checks();
    decide_checks();
    std::printf(failures ? "vad_check: %d failures\n" : "vad_check: all checks held\n", failures);
    return failures ? 1 : 0;
}
