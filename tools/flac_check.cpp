// Stand-alone host check of the FLAC reader: the frame index (csrc/flac_format.h) and the per-frame decode (csrc/flac_decode.h) - the
// code the library and its kernels are built from - run on the CPU over the files named on the command line.  Per file one line: frames,
// samples, the MD5 of the decoded interleaved little-endian PCM and whether it equals STREAMINFO's signature.
//   --flip [--stride N]   decode every frame again with each single bit (every N-th) of the frame flipped in turn, the CRC verdicts
//                         ignored, from a heap copy of exactly the frame's bytes into buffers of exactly the sizes the decoder was
//                         told: what is exercised is the bounds logic.  Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/flac_check.cpp -o flac_check
// Exit status 0 when every file indexed, decoded and matched its MD5.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "flac_decode.h"

namespace {

struct Md5 {
    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    static uint32_t rol(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
    void block(const uint8_t* p) {
        static const int S[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20,
                                  4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
        static uint32_t K[64];
        static bool init = false;
        if (!init) {
            for (int i = 0; i < 64; ++i) K[i] = (uint32_t)(4294967296.0 * __builtin_fabs(__builtin_sin((double)(i + 1))));
            init = true;
        }
        uint32_t m[16];
        for (int i = 0; i < 16; ++i) m[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
        for (int i = 0; i < 64; ++i) {
            uint32_t f;
            int g;
            if (i < 16) f = (b & c) | (~b & d), g = i;
            else if (i < 32) f = (d & b) | (~d & c), g = (5 * i + 1) & 15;
            else if (i < 48) f = b ^ c ^ d, g = (3 * i + 5) & 15;
            else f = c ^ (b | ~d), g = (7 * i) & 15;
            const uint32_t t = d;
            d = c;
            c = b;
            b = b + rol(a + f + K[i] + m[g], S[i]);
            a = t;
        }
        h[0] += a, h[1] += b, h[2] += c, h[3] += d;
    }
    std::string of(const std::vector<uint8_t>& data) {
        std::vector<uint8_t> v(data);
        const uint64_t bits = (uint64_t)data.size() * 8;
        v.push_back(0x80);
        while (v.size() % 64 != 56) v.push_back(0);
        for (int i = 0; i < 8; ++i) v.push_back((uint8_t)(bits >> (8 * i)));
        for (size_t i = 0; i < v.size(); i += 64) block(&v[i]);
        char out[33];
        for (int i = 0; i < 16; ++i) snprintf(out + 2 * i, 3, "%02x", (h[i / 4] >> (8 * (i % 4))) & 0xFF);
        return out;
    }
};

// one frame -> its samples (block size x channels, interleaved) in `out` (room for exactly room * channels values); false: refused
bool decode_frame(const uint8_t* p, int64_t len, int channels, int64_t room, bool check_crc8, std::vector<int32_t>* out) {
    FlacFrameHeader h;
    if (!flac_parse_header(p, len, &h, check_crc8) || h.block_size > room) return false;
    const int64_t words = flac_frame_words(channels, h.block_size);
    std::unique_ptr<int32_t[]> w(new int32_t[words]());  // exactly the words the decoder is told it has
    if (flac_entropy_frame(p, len, channels, room, words, w.get(), 1, check_crc8)) return false;
    for (int c = 0; c < channels; ++c) flac_restore_channel(w.get(), 1, c);
    out->assign((size_t)h.block_size * channels, 0);
    for (int i = 0; i < h.block_size; ++i)
        for (int c = 0; c < channels; ++c) (*out)[(size_t)i * channels + c] = flac_output_sample(w.get(), 1, c, i);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    bool flip = false;
    long stride = 1;
    std::vector<std::string> files;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--flip")) flip = true;
        else if (!strcmp(argv[i], "--stride") && i + 1 < argc) stride = std::max(1L, atol(argv[++i]));
        else files.push_back(argv[i]);
    }
    if (files.empty()) {
        fprintf(stderr, "usage: flac_check [--flip [--stride N]] FILE...\n");
        return 2;
    }
    int failed = 0;
    for (const std::string& path : files) {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) {
            printf("%s: cannot open\n", path.c_str());
            ++failed;
            continue;
        }
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
        fclose(f);
        size_t pos = 4;
        bool last = false, ok = data.size() >= 42 && !memcmp(data.data(), "fLaC", 4) && (data[4] & 0x7F) == 0;
        while (ok && !last) {
            if (pos + 4 > data.size()) ok = false;
            else {
                last = data[pos] & 0x80;
                pos += 4 + (((size_t)data[pos + 1] << 16) | ((size_t)data[pos + 2] << 8) | data[pos + 3]);
                ok = pos <= data.size();
            }
        }
        if (!ok) {
            printf("%s: not a FLAC stream with a whole metadata chain\n", path.c_str());
            ++failed;
            continue;
        }
        const uint8_t* si = &data[8];
        const int rate = (si[10] << 12) | (si[11] << 4) | (si[12] >> 4), channels = ((si[12] >> 1) & 7) + 1, bits = (((si[12] & 1) << 4) | (si[13] >> 4)) + 1;
        const int64_t total = ((int64_t)(si[13] & 15) << 32) | ((int64_t)si[14] << 24) | (si[15] << 16) | (si[16] << 8) | si[17];
        char want[33];
        for (int i = 0; i < 16; ++i) snprintf(want + 2 * i, 3, "%02x", si[18 + i]);
        // (a heap copy of exactly the audio bytes: a read behind them is the sanitizer's to report)
        const int64_t n = (int64_t)(data.size() - pos);
        std::unique_ptr<uint8_t[]> audio(new uint8_t[n > 0 ? n : 1]);
        memcpy(audio.get(), data.data() + pos, (size_t)n);
        int64_t frames = 0, samples = 0, bad = 0;
        int rc = bits == 16 ? flac_index(audio.get(), n, rate, channels, bits, nullptr, 0, &frames, &samples, &bad) : -1;
        std::vector<int32_t> index((size_t)frames * 3 + 1);
        if (rc == 0) rc = flac_index(audio.get(), n, rate, channels, bits, index.data(), frames, &frames, &samples, &bad);
        if (rc != 0 || (total && total != samples)) {
            printf("%s: index refused (%d) at byte offset %lld; %lld samples found, STREAMINFO says %lld, %d bits\n", path.c_str(), rc, (long long)bad,
                   (long long)samples, (long long)total, bits);
            ++failed;
            continue;
        }
        std::vector<uint8_t> pcm((size_t)samples * channels * 2);
        std::vector<int32_t> out;
        bool good = true;
        long flips = 0;
        for (int64_t k = 0; k < frames && good; ++k) {
            const int64_t off = index[3 * k], len = index[3 * k + 1], first = index[3 * k + 2];
            good = decode_frame(audio.get() + off, len, channels, samples - first, true, &out) && (int64_t)out.size() <= (samples - first) * channels;
            if (!good) break;
            for (size_t j = 0; j < out.size(); ++j) {
                pcm[2 * ((size_t)first * channels + j)] = (uint8_t)(out[j] & 0xFF);
                pcm[2 * ((size_t)first * channels + j) + 1] = (uint8_t)((out[j] >> 8) & 0xFF);
            }
            if (flip) {
                std::unique_ptr<uint8_t[]> copy(new uint8_t[len]);
                std::vector<int32_t> scratch;
                for (int64_t bit = 0; bit < len * 8; bit += stride) {
                    memcpy(copy.get(), audio.get() + off, (size_t)len);
                    copy[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
                    (void)decode_frame(copy.get(), len, channels, samples - first, false, &scratch);
                    ++flips;
                }
            }
        }
        const std::string got = good ? Md5().of(pcm) : "";
        const bool match = good && got == want;
        printf("%s: %lld frames, %lld samples, %d ch, %d Hz, md5 %s %s", path.c_str(), (long long)frames, (long long)samples, channels, rate,
               good ? got.c_str() : "(a frame did not decode)", match ? "OK" : "MISMATCH");
        if (flip) printf(", %ld flipped decodes", flips);
        printf("\n");
        if (!match) ++failed;
    }
    return failed ? 1 : 0;
}
