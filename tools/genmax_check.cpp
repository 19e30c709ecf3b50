// Stand-alone host check of the fused generator tail's host side (csrc/genmax.hip: decide_genmax, pack_genmax, pack_genmax_x3):
// every buffer a heap block of exactly the size include/cassnat_hip_genmax.h states, so that a sanitizer sees any read or write past
// one - W [V][256] and b [V] read, waves * vtw * 16 KiB (split: 32 KiB) of fragments and waves * vtw * 32 biases written - at the
// vocabulary sizes where the tile counts change (1, 32, 33, 128, 129, 257, 384, 1028, 4234, 6143, 6144); every refusal of
// decide_genmax for sizes from INT32_MIN to INT32_MAX, which must come back with a message and without arithmetic overflow; and the
// form of every accepted (M, V): LDS bytes within 160 KiB, grid * rows per workgroup >= M.  No device call is made.
// Meant to be built with sanitizers on the host side (the kernels of genmax.hip are compiled but never launched):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -x hip tools/genmax_check.cpp cassnat_asr_public_amd/csrc/genmax.hip -o genmax_check
// Exit status 0 when every check held.
#include <climits>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>

#include "../cassnat_asr_public_amd/csrc/kernels.h"

static std::string last_error;
void cn_set_error(const std::string& msg) { last_error = msg; }

namespace {

int failures = 0;

void fail(const char* what, long long a, long long b) {
    std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
    ++failures;
}

void pack_case(int V, bool x3) {
    const int waves = x3 ? 8 : 4, vtw = x3 ? genmax_x3_vtw(V) : genmax_vtw(V);
    const size_t wn = (size_t)waves * vtw * 16 * (x3 ? 1024 : 512), bn = (size_t)waves * vtw * 32;
    std::unique_ptr<float[]> w(new float[(size_t)V * 256]), b(new float[V]), bout(new float[bn]);
    std::unique_ptr<uint16_t[]> wout(new uint16_t[wn]);
    for (size_t i = 0; i < (size_t)V * 256; ++i) w[i] = 0.001f * (float)((i * 2654435761u) % 2001) - 1.f;
    for (int v = 0; v < V; ++v) b[v] = 0.25f * (float)(v % 7) - 0.5f;
    (x3 ? pack_genmax_x3 : pack_genmax)(w.get(), b.get(), V, wout.get(), bout.get());
    // spot checks of the stated layout: entry v, column k
    for (int v : {0, V / 2, V - 1, V, waves * vtw * 32 - 1})
        for (int k : {0, 7, 8, 255}) {
            const int tile = v / 32, ks = k / 16, lane = (v & 31) + 32 * ((k >> 3) & 1), j = k & 7;
            const size_t o = x3 ? ((((size_t)tile * 16 + ks) * 2) * 64 + lane) * 8 + j : (((size_t)tile * 16 + ks) * 64 + lane) * 8 + j;
            const uint16_t want = v < V ? cn_host_op16(w[(size_t)v * 256 + k]) : 0;
            if (v < waves * vtw * 32 && wout[o] != want) fail("packed weight", v, k);
            if (x3 && v >= V && v < waves * vtw * 32 && wout[o + 512] != 0) fail("padded lo half", v, k);
        }
    for (size_t i = 0; i < bn; ++i)
        if (i < (size_t)V ? bout[i] != b[i] : !(std::isinf(bout[i]) && bout[i] < 0)) fail("packed bias", V, (long long)i);
}

void decide_cases() {
    static const int dummy = 0;
    const int sizes[] = {INT_MIN, INT_MIN + 1, -6145, -1000, -128, -127, -1, 0, 1, 31, 32, 33, 64, 65, 6143, 6144, 6145, 8192, 8193,
                         1 << 20, INT_MAX - 31, INT_MAX - 1, INT_MAX};
    for (int x3 = 0; x3 < 2; ++x3)
        for (int V : sizes)
            for (int M : sizes)
                for (int kind = 0; kind < 3; ++kind) {
                    GenmaxArgs a;
                    a.x3 = x3 != 0;
                    a.h = &dummy;
                    a.M = M;
                    a.V = V;
                    a.d = 256;
                    if (kind == GENMAX_GATHER) {
                        a.tgt = &dummy;
                        a.tgt_lp = reinterpret_cast<float*>(const_cast<int*>(&dummy));
                        a.tgt_U = a.tgt_ld = 1;
                    } else {
                        a.arg = const_cast<int*>(&dummy);
                        if (kind == GENMAX_ARGMAX_LSE) a.maxlp = reinterpret_cast<float*>(const_cast<int*>(&dummy));
                    }
                    GenmaxForm f;
                    last_error.clear();
                    const int rc = decide_genmax(a, &f, "check", false);
                    const bool ok = V >= 1 && V <= 6144 && M >= 0;
                    if ((rc == 0) != ok) fail("decide_genmax accepts", M, V);
                    if (rc != 0 && last_error.rfind("check: ", 0) != 0) fail("refusal without the caller's name", M, V);
                    if (rc != 0) continue;
                    if (f.kind != kind || f.x3 != a.x3 || f.vtw != (x3 ? genmax_x3_vtw(V) : genmax_vtw(V))) fail("form", M, V);
                    if (M == 0 ? f.mt != 0 || f.grid != 0 : (f.mt < 1 || f.mt > 2 || (long long)f.grid * 32 * f.mt < M || f.lds > 160 * 1024 || f.lds <= 0))
                        fail("launch shape", M, V);
                }
}

}  // namespace

int main() {
    for (int V : {1, 32, 33, 128, 129, 257, 384, 1028, 4234, 6143, 6144}) {
        pack_case(V, false);
        pack_case(V, true);
    }
    decide_cases();
    std::printf(failures ? "%d checks failed\n" : "all checks held\n", failures);
    return failures ? 1 : 0;
}
