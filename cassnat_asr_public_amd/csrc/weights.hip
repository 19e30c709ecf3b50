// The weight packer: lays every tensor of the model out in ONE device blob (so that a broadcast or a second handle carries all
// of it) in the forms the kernels read - plain matrices, fragment streams, row-chain streams, e4m3 and split-bf16 copies - and
// hands the handle its views into that blob.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "model.h"

namespace cn_host {
namespace {

inline uint16_t f32_to_bf16_host(float f) { return cn_host_op16(f); }  // (the engine's 16-bit operand: common.h)

// split-bf16 forms: the (hi, lo) pair of a float - hi = bf16(v), lo = bf16(v - hi) - stored `lo_off` bytes apart
inline void put_hi_lo(unsigned char* hi_at, size_t lo_off, float v) {
    const uint16_t hi = f32_to_bf16_host(v);
    const uint32_t hb = (uint32_t)hi << 16;
    float hf;
    std::memcpy(&hf, &hb, 4);
    const uint16_t lo = f32_to_bf16_host(v - hf);
    std::memcpy(hi_at, &hi, 2);
    std::memcpy(hi_at + lo_off, &lo, 2);
}

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
struct Packer {
    cn_model* m;
    bool fill;                        // false: layout only (weights arrive by broadcast)
    unsigned char* base;              // the device blob the views point into (null: the first pass, whose views are unused)
    std::vector<unsigned char> host;  // staging image of the blob, indexed by offset
    size_t off = 256;  // offset 0 is reserved: no view is ever the blob's own address
    std::string missing;

    Packer(cn_model* m_, bool fill_, unsigned char* base_) : m(m_), fill(fill_), base(base_) {}
    // the device address of a reserved offset: every view is made through this, so none exists without its base
    template <typename P> P* view(size_t at) const { return reinterpret_cast<P*>(reinterpret_cast<uintptr_t>(base) + at); }

    size_t reserve(size_t bytes) {
        const size_t at = off;
        off = (off + bytes + 255) & ~(size_t)255;
        if (fill && host.size() < off) host.resize(off);
        return at;
    }
    const HostTensor* find(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = m->host.find(name);
        if (it == m->host.end()) {
            it = m->host.find("module." + name);
            if (it == m->host.end()) {
                if (missing.size() < 400) missing += name + " ";
                return nullptr;
            }
        }
        if (it->second.shape != std::vector<int64_t>(shape)) {
            missing += name + "(shape) ";
            return nullptr;
        }
        return &it->second;
    }
    void put_elem(size_t at, size_t idx, float v) {
        if (m->prec == CN_PREC_F32)
            std::memcpy(&host[at + idx * 4], &v, 4);
        else if (m->prec == CN_PREC_X3)  // split-bf16: hi / lo halves of the element's 32-group (every packed row is a
            put_hi_lo(&host[at + cn_split_off(idx)], 64, v);  // multiple of 32 long, so flat groups never straddle rows)
        else {
            const uint16_t h = f32_to_bf16_host(v);
            std::memcpy(&host[at + idx * 2], &h, 2);
        }
    }
    // fp32 vector made by concatenating several named vectors
    float* vec(std::initializer_list<std::string> names, int64_t each) {
        const size_t at = reserve(names.size() * each * 4);
        if (fill) {
            size_t k = 0;
            for (auto& n : names) {
                const HostTensor* t = find(n, {each});
                if (t) std::memcpy(&host[at + k * each * 4], t->data.data(), each * 4);
                ++k;
            }
        }
        return view<float>(at);
    }
    // fp8 copy of a packed Linear (same row order as `linear` built it from `prefixes`): one power-of-two scale per tensor,
    // the largest that keeps max|w| * scale <= 448
    void quant8(Linear& l, std::initializer_list<std::string> prefixes, int64_t rows_each) {
        const size_t at = reserve((size_t)l.N * l.K);
        const size_t sat = reserve(4);
        if (fill) {
            float mx = 0.f;
            for (auto& pfx : prefixes) {
                const HostTensor* t = find(pfx + ".weight", {rows_each, (int64_t)l.K});
                if (t)
                    for (float v : t->data) mx = std::max(mx, std::fabs(v));
            }
            const float scale = std::ldexp(1.f, cn_e4m3_exp(mx));
            size_t r0 = 0;
            for (auto& pfx : prefixes) {
                const HostTensor* t = find(pfx + ".weight", {rows_each, (int64_t)l.K});
                if (t)
                    for (int64_t i = 0; i < rows_each * l.K; ++i) host[at + r0 * l.K + i] = cn_f32_to_e4m3_host(t->data[i] * scale);
                r0 += rows_each;
            }
            const float inv = 1.f / scale;
            std::memcpy(&host[sat], &inv, 4);
        }
        l.W8 = view<void>(at);
        l.w8_inv = view<float>(sat);
    }
    // [sum rows][K] matrix in model precision from several [rows][K] matrices, optional column permutation
    Linear linear(std::initializer_list<std::string> prefixes, int64_t rows_each, int64_t K,
                  const std::vector<int>* colperm = nullptr) {
        Linear l;
        l.N = (int)(prefixes.size() * rows_each);
        l.K = (int)K;
        const size_t at = reserve((size_t)l.N * K * m->es);
        if (fill) {
            size_t r0 = 0;
            for (auto& pfx : prefixes) {
                const HostTensor* t = find(pfx + ".weight", {rows_each, K});
                if (t) {
                    for (int64_t r = 0; r < rows_each; ++r)
                        for (int64_t c = 0; c < K; ++c) {
                            const int64_t src_c = colperm ? (*colperm)[c] : c;
                            put_elem(at, (r0 + r) * K + c, t->data[r * K + src_c]);
                        }
                }
                r0 += rows_each;
            }
        }
        l.W = view<void>(at);
        if (m->prec == CN_PREC_X3 && proj_x3_applies(l.N, l.K)) {  // the same matrix as the projection kernel's fragment stream
            const size_t pat = reserve((size_t)l.N * 1024);
            if (fill) {
                size_t r0 = 0;
                for (auto& pfx : prefixes) {
                    const HostTensor* t = find(pfx + ".weight", {rows_each, K});
                    if (t)
                        for (int64_t r = 0; r < rows_each; ++r)
                            for (int64_t c = 0; c < K; ++c)
                                put_hi_lo(&host[pat + proj_x3_off((int)(r0 + r), (int)c)], 1024, t->data[r * K + (colperm ? (*colperm)[c] : c)]);
                    r0 += rows_each;
                }
            }
            l.px3 = view<void>(pat);
        }
        size_t bat = reserve((size_t)l.N * 4);
        if (fill) {
            size_t k = 0;
            for (auto& pfx : prefixes) {
                const HostTensor* t = find(pfx + ".bias", {rows_each});
                if (t) std::memcpy(&host[bat + k * rows_each * 4], t->data.data(), rows_each * 4);
                ++k;
            }
        }
        l.b = view<float>(bat);
        return l;
    }
    // nn.Conv1d(kernel 1) weight [rows][K][1] as a Linear
    Linear pointwise(const std::string& prefix, int64_t rows, int64_t K) {
        Linear l;
        l.N = (int)rows;
        l.K = (int)K;
        const size_t at = reserve((size_t)rows * K * m->es);
        if (fill) {
            const HostTensor* t = find(prefix + ".weight", {rows, K, 1});
            if (t)
                for (int64_t i = 0; i < rows * K; ++i) put_elem(at, i, t->data[i]);
        }
        l.W = view<void>(at);
        l.b = vec({prefix + ".bias"}, rows);
        return l;
    }
    // fp32 copy of a named tensor of any shape with n elements
    float* raw(const std::string& name, std::initializer_list<int64_t> shape, int64_t n) {
        const size_t at = reserve((size_t)n * 4);
        if (fill) {
            const HostTensor* t = find(name, shape);
            if (t) std::memcpy(&host[at], t->data.data(), (size_t)n * 4);
        }
        return view<float>(at);
    }
    // plain (unfused) feed-forward pair
    void ffn_plain(Linear& w1, Linear& w2, const std::string& p, int64_t dff, int64_t d) {
        w1 = linear({p + ".w_1"}, dff, d);
        w2 = linear({p + ".w_2"}, d, dff);
    }
    ConvMod conv_module(const std::string& p, int64_t d, int64_t k) {
        ConvMod c;
        c.pw1 = pointwise(p + ".pointwise_conv1", 2 * d, d);
        c.dw_w = raw(p + ".depthwise_conv.weight", {d, 1, k}, d * k);
        c.dw_b = vec({p + ".depthwise_conv.bias"}, d);
        c.gn_w = vec({p + ".norm.weight"}, d);
        c.gn_b = vec({p + ".norm.bias"}, d);
        c.pw2 = pointwise(p + ".pointwise_conv2", d, d);
        c.k = (int)k;
        return c;
    }
    // relative-position self attention: fused Q|K|V, output projection, u / v, and P = table . W_pos^T (the position rows
    // are a frozen sinusoid table in the checkpoint, so their projection is a constant of the layer)
    void rel_attn(Layer& L, const std::string& att, const std::string& table, int64_t R, int64_t d, int64_t H) {
        L.has_self = true;
        L.qkv = linear({att + ".linears.0", att + ".linears.1", att + ".linears.2"}, d, d);
        L.self_o = linear({att + ".linears.3"}, d, d);
        L.pos_u = raw(att + ".pos_bias_u", {H, d / H}, d);
        L.pos_v = raw(att + ".pos_bias_v", {H, d / H}, d);
        const int64_t nr = 2 * R + 1;
        const size_t at = reserve((size_t)nr * d * 4);
        if (fill) {
            const HostTensor* tb = find(table, {nr, d});
            const HostTensor* wp = find(att + ".linear_pos.weight", {d, d});
            if (tb && wp)
                for (int64_t r = 0; r < nr; ++r)
                    for (int64_t o = 0; o < d; ++o) {
                        double acc = 0.0;
                        for (int64_t i = 0; i < d; ++i) acc += (double)tb->data[r * d + i] * (double)wp->data[o * d + i];
                        const float v = (float)acc;
                        std::memcpy(&host[at + (r * d + o) * 4], &v, 4);
                    }
        }
        L.pos_proj = view<float>(at);
        L.rel_R = (int)R;
    }
    // conformer self-attention block (fanat_conformer_blocks.py:9-38): feed_forward1, self_attn, conv_module, feed_forward2
    Layer conformer_layer(const std::string& p, const std::string& table, int64_t dff, int64_t k, int64_t R, int64_t d, int64_t H,
                          int nnorm) {
        Layer L;
        L.conformer = true;
        rel_attn(L, p + ".self_attn", table, R, d, H);
        ffn_plain(L.w1, L.w2, p + ".feed_forward1", dff, d);
        L.conv = conv_module(p + ".conv_module", d, k);
        ffn_plain(L.ff2_w1, L.ff2_w2, p + ".feed_forward2", dff, d);
        for (int i = 0; i < nnorm; ++i) L.n[i] = norm(p + ".sublayer." + std::to_string(i) + ".norm", d);
        return L;
    }
    // feed-forward weights: fragment streams for the fused kernel when it applies, plain matrices otherwise (L.ff_swish set
    // before: a Swish layer's split-bf16 stream is the plain split form's, never the mixed arithmetic's)
    void ffn(Layer& L, const std::string& p, int64_t dff, int64_t d) {
        const bool fused = m->prec == CN_PREC_BF16 && d == 256 && dff % 128 == 0 && dff <= 2048;
        if (m->prec == CN_PREC_X3 && ffn_x3_applies((int)d, (int)dff)) {
            const size_t ax = reserve(ffn_x3_stream_bytes((int)dff));
            if (fill) {
                const HostTensor* t1 = find(p + ".feed_forward.w_1.weight", {dff, d});
                const HostTensor* t2 = find(p + ".feed_forward.w_2.weight", {d, dff});
                if (t1 && t2)
                    pack_ffn_x3(t1->data.data(), t2->data.data(), (int)dff, reinterpret_cast<uint16_t*>(&host[ax]), !L.ff_swish && ffn_mix_applies());
            }
            L.wx3 = view<void>(ax);
        } else if (fused) {
            const size_t a1 = reserve((size_t)dff * d * 2), a2 = reserve((size_t)dff * d * 2);
            if (fill) {
                const HostTensor* t1 = find(p + ".feed_forward.w_1.weight", {dff, d});
                const HostTensor* t2 = find(p + ".feed_forward.w_2.weight", {d, dff});
                if (t1) pack_ffn_w1(t1->data.data(), (int)dff, reinterpret_cast<uint16_t*>(&host[a1]));
                if (t2) pack_ffn_w2(t2->data.data(), (int)dff, reinterpret_cast<uint16_t*>(&host[a2]));
            }
            L.w1p = view<void>(a1);
            L.w2p = view<void>(a2);
        } else {
            L.w1 = linear({p + ".feed_forward.w_1"}, dff, d);
            L.w2 = linear({p + ".feed_forward.w_2"}, d, dff);
            return;
        }
        // (either stream: w1 / w2 hold the shapes and the biases only)
        L.w1.N = (int)dff;
        L.w1.K = (int)d;
        L.w1.b = vec({p + ".feed_forward.w_1.bias"}, dff);
        L.w2.N = (int)d;
        L.w2.K = (int)dff;
        L.w2.b = vec({p + ".feed_forward.w_2.bias"}, d);
    }
    bool chain_ok(int64_t d, int64_t dff) const {
        return m->prec == CN_PREC_BF16 && d == 256 && dff % 32 == 0 && dff <= 2048;
    }
    // One row-chain stream by tensor names: out-projection, FFN with its pre-norm, then the norm and the concatenated
    // projections of whatever consumes the stream next.  In a conformer sublayer group (fanat_conformer_blocks.py:26-38) the
    // output projection / tail may be a pointwise convolution ([rows][d][1]) and the feed-forward is a macaron half - Swish,
    // and its 0.5 residual scale folded into w_2 and b_2 (a power of two: exact in bf16)
    struct ChainSpec {
        std::string wo;          // "" or prefix of a [d][d] Linear / [d][d][1] pointwise conv (+ ".bias")
        bool wo_conv = false;
        std::string ln1, ffn;    // FFN pre-norm and prefix (".w_1" / ".w_2"), "" = none
        int64_t dff = 0;
        float ffn_scale = 1.f;
        bool swish = false;      // the FFN's activation (else ReLU)
        bool f8 = false;         // the FFN's units in e4m3 (chain.hip, F8 form)
        std::string nln;         // next norm ("" = none)
        std::vector<std::string> tails;  // each a prefix of [rows][d](,1) weights
        int64_t tail_rows = 0;   // rows per tail tensor
        bool tail_conv = false;
    };
    // Seven spare units follow the stream: the kernel's dummy refills past the end read them.
    ChainRef chain_stream(const ChainSpec& c, int64_t d) {
        ChainRef r;
        const int tail_n = (int)(c.tails.size() * c.tail_rows);
        const size_t units = chain_stream_units(!c.wo.empty(), (int)c.dff, tail_n, c.f8);
        const size_t aw = reserve((units + 7) * CHAIN_UNIT_BYTES), at = reserve((size_t)CHAIN_TAB_FLOATS * 4);
        const size_t aq = c.f8 ? reserve(16) : 0;
        if (fill) {
            ChainWeights w;
            bool ok = true;
            auto get = [&](const std::string& n, std::initializer_list<int64_t> shape) -> const float* {
                const HostTensor* t = find(n, shape);
                if (!t) ok = false;
                return t ? t->data.data() : nullptr;
            };
            std::vector<float> w2s, b2s;
            if (!c.wo.empty()) {
                w.wo = c.wo_conv ? get(c.wo + ".weight", {d, d, 1}) : get(c.wo + ".weight", {d, d});
                w.bo = get(c.wo + ".bias", {d});
            }
            if (c.dff) {
                w.ln1_a = get(c.ln1 + ".a_2", {d});
                w.ln1_b = get(c.ln1 + ".b_2", {d});
                w.w1 = get(c.ffn + ".w_1.weight", {c.dff, d});
                w.b1 = get(c.ffn + ".w_1.bias", {c.dff});
                w.w2 = get(c.ffn + ".w_2.weight", {d, c.dff});
                w.b2 = get(c.ffn + ".w_2.bias", {d});
                if (w.w2 && w.b2 && c.ffn_scale != 1.f) {
                    w2s.assign(w.w2, w.w2 + (size_t)d * c.dff);
                    b2s.assign(w.b2, w.b2 + d);
                    for (auto& v : w2s) v *= c.ffn_scale;
                    for (auto& v : b2s) v *= c.ffn_scale;
                    w.w2 = w2s.data();
                    w.b2 = b2s.data();
                }
            }
            if (!c.nln.empty()) {
                w.nln_a = get(c.nln + ".a_2", {d});
                w.nln_b = get(c.nln + ".b_2", {d});
            }
            std::vector<float> tw((size_t)tail_n * d), tb((size_t)tail_n);
            size_t k = 0;
            for (auto& tp : c.tails) {
                const float* a = c.tail_conv ? get(tp + ".weight", {c.tail_rows, d, 1}) : get(tp + ".weight", {c.tail_rows, d});
                const float* b = get(tp + ".bias", {c.tail_rows});
                if (a && b) {
                    std::memcpy(&tw[k * c.tail_rows * d], a, (size_t)c.tail_rows * d * 4);
                    std::memcpy(&tb[k * c.tail_rows], b, (size_t)c.tail_rows * 4);
                }
                ++k;
            }
            w.wt = tw.data();
            w.bt = tb.data();
            w.dff = (int)c.dff;
            w.tail_n = tail_n;
            if (ok) pack_chain(w, reinterpret_cast<uint16_t*>(&host[aw]), reinterpret_cast<float*>(&host[at]),
                               c.f8 ? reinterpret_cast<int*>(&host[aq]) : nullptr);
        }
        r.w = view<void>(aw);
        r.tab = view<float>(at);
        r.f8q = c.f8 ? view<int>(aq) : nullptr;
        r.dff = (int)c.dff;
        r.tail_n = tail_n;
        r.has_wo = !c.wo.empty();
        r.has_next = !c.nln.empty();
        r.swish = c.swish;
        return r;
    }
    // The transformer layers' form of it: out-projection `wo` ("" = none), the ReLU FFN of layer `p` with pre-norm `ln1` (dff 0 =
    // none), then norm `nln` ("" = nothing follows) and the projections `tails` (each [d][d])
    ChainRef chain(const std::string& wo, const std::string& ln1, const std::string& p, int64_t dff, const std::string& nln,
                   std::vector<std::string> tails, int64_t d, bool f8 = false) {
        ChainSpec c;
        c.wo = wo;
        c.ln1 = ln1;
        c.ffn = p + ".feed_forward";
        c.dff = dff;
        c.f8 = f8;
        c.nln = nln;
        c.tails = std::move(tails);
        c.tail_rows = d;
        return chain_stream(c, d);
    }
    // generator: the plain matrix (beam search / capture) plus the fused-argmax fragment stream when it applies
    Linear generator(const std::string& prefix, int64_t V, int64_t d) {
        Linear l = linear({prefix}, V, d);
        if (genmax_applies(m->prec, (int)d, (int)V)) {
            const bool x3 = m->prec == CN_PREC_X3;
            const int vtw = x3 ? genmax_x3_vtw((int)V) : genmax_vtw((int)V);
            const size_t aw = reserve(x3 ? (size_t)8 * vtw * 32 * 1024 : (size_t)4 * vtw * 16 * 1024);
            const size_t ab = reserve((size_t)(x3 ? 8 : 4) * vtw * 32 * 4);
            if (fill) {
                const HostTensor* tw = find(prefix + ".weight", {V, d});
                const HostTensor* tb = find(prefix + ".bias", {V});
                if (tw && tb)
                    (x3 ? pack_genmax_x3 : pack_genmax)(tw->data.data(), tb->data.data(), (int)V, reinterpret_cast<uint16_t*>(&host[aw]),
                                                        reinterpret_cast<float*>(&host[ab]));
            }
            l.gm_w = view<void>(aw);
            l.gm_b = view<float>(ab);
        }
        return l;
    }
    Norm norm(const std::string& prefix, int64_t d) {
        Norm n;
        n.a = vec({prefix + ".a_2"}, d);
        n.b = vec({prefix + ".b_2"}, d);
        return n;
    }
};

// One pass over the model in blob order: reserves every region (the order of the reserve calls IS the layout, a pure function
// of the configuration and the engine), fills the staging image when pk.fill, and sets every weight view of the handle
void pack_model(cn_model* m, Packer& pk) {
    const cn_config& c = m->cfg;
    const int64_t d = c.d_model, V = c.vocab_size, C = c.d_model;
    const int64_t F2 = m->F2;
    // cfg.ast == 2: the TransformerLM that ranks ESA samples (src/models/lm.py): token embedding, encoder stack, generator
    const bool lm = c.ast == 2;

    // conv1: (C,1,3,3) -> [tap][C] fp32
    if (!lm) {
        const size_t at = pk.reserve(9 * C * 4);
        if (pk.fill) {
            const HostTensor* t = pk.find("src_embed.conv.0.weight", {C, 1, 3, 3});
            if (t)
                for (int64_t ch = 0; ch < C; ++ch)
                    for (int tap = 0; tap < 9; ++tap)
                        std::memcpy(&pk.host[at + (tap * C + ch) * 4], &t->data[ch * 9 + tap], 4);
        }
        m->conv1_w = pk.view<float>(at);
        m->conv1_b = pk.vec({"src_embed.conv.0.bias"}, C);
    }
    // conv2: (Co,Ci,3,3) -> [Co][(kh,kw,ci)]
    if (!lm) {
        m->conv2.N = (int)C;
        m->conv2.K = (int)(9 * C);
        const size_t at = pk.reserve((size_t)C * 9 * C * m->es);
        if (pk.fill) {
            const HostTensor* t = pk.find("src_embed.conv.2.weight", {C, C, 3, 3});
            if (t)
                for (int64_t co = 0; co < C; ++co)
                    for (int64_t ci = 0; ci < C; ++ci)
                        for (int tap = 0; tap < 9; ++tap)
                            pk.put_elem(at, co * 9 * C + tap * C + ci, t->data[(co * C + ci) * 9 + tap]);
        }
        m->conv2.W = pk.view<void>(at);
        if (conv2_x3_applies(m->prec, (int)C, (int)C)) {
            const size_t plane = (size_t)C * 9 * C * 2, pat = pk.reserve(2 * plane);
            if (pk.fill) {
                const HostTensor* t = pk.find("src_embed.conv.2.weight", {C, C, 3, 3});
                if (t)
                    for (int64_t co = 0; co < C; ++co)
                        for (int64_t ci = 0; ci < C; ++ci)
                            for (int tap = 0; tap < 9; ++tap)
                                put_hi_lo(&pk.host[pat + (size_t)(co * 9 * C + tap * C + ci) * 2], plane, t->data[(co * C + ci) * 9 + tap]);
            }
            m->conv2_x3w = pk.view<void>(pat);
        }
        if (conv2_mix_applies(m->prec, (int)C, (int)C)) {
            const size_t pat = pk.reserve((size_t)C * 9 * C * 4), qat = pk.reserve(16);
            if (pk.fill) {
                const HostTensor* t = pk.find("src_embed.conv.2.weight", {C, C, 3, 3});
                if (t) pack_conv2_mix(t->data.data(), (int)C, 9 * C, 1, 9, &pk.host[pat], reinterpret_cast<int*>(&pk.host[qat]));
            }
            m->conv2_mixw = pk.view<void>(pat);
            m->conv2_mixq = pk.view<int>(qat);
        }
        if (m->fp8_enc && (m->fp8_scope & CN_FP8_CONV2) && conv2_f8_applies((int)C, (int)C)) {  // config 5: the second convolution on e4m3 operands (conv2.hip, F8)
            const size_t fat = pk.reserve((size_t)C * 9 * C), qat = pk.reserve(16);
            if (pk.fill) {
                const HostTensor* t = pk.find("src_embed.conv.2.weight", {C, C, 3, 3});
                if (t) {
                    const int lg = pack_conv2_f8(t->data.data(), (int)C, 9 * C, 1, 9, &pk.host[fat]);
                    const int q[4] = {127 - lg, 127 - (int)std::lround(std::log2(FP8_S_IMG)), 0, 0};
                    std::memcpy(&pk.host[qat], q, 16);
                }
            }
            m->conv2_f8w = pk.view<void>(fat);
            m->conv2_f8q = pk.view<int>(qat);
        }
        m->conv2.b = pk.vec({"src_embed.conv.2.bias"}, C);
    }
    if (!lm) {
        // |conv1 out| <= fmax A1 + B1 and |conv2 out| <= |conv1 out| A2 + B2 with A = the largest row sum of |weights|, B = the
        // largest |bias|: the feature magnitude that keeps both under half of 65504 (0: weights unknown here - no check)
        const size_t at = pk.reserve(16);
        if (pk.fill) {
            float lim = 0.f;
            const HostTensor* w1 = pk.find("src_embed.conv.0.weight", {C, 1, 3, 3});
            const HostTensor* b1 = pk.find("src_embed.conv.0.bias", {C});
            const HostTensor* w2 = pk.find("src_embed.conv.2.weight", {C, C, 3, 3});
            const HostTensor* b2 = pk.find("src_embed.conv.2.bias", {C});
            if (w1 && b1 && w2 && b2) {
                double A1 = 0, B1 = 0, A2 = 0, B2 = 0;
                for (int64_t ch = 0; ch < C; ++ch) {
                    double r1 = 0, r2 = 0;
                    for (int k = 0; k < 9; ++k) r1 += std::fabs((double)w1->data[ch * 9 + k]);
                    for (int64_t k = 0; k < 9 * C; ++k) r2 += std::fabs((double)w2->data[ch * 9 * C + k]);
                    A1 = std::max(A1, r1);
                    A2 = std::max(A2, r2);
                    B1 = std::max(B1, std::fabs((double)b1->data[ch]));
                    B2 = std::max(B2, std::fabs((double)b2->data[ch]));
                }
#ifdef CN_OP16_F16
                const double half_max = 65504.0 / 2;
                const double c1 = std::min(half_max, A2 > 0 ? (half_max - B2) / A2 : half_max);  // the bound on conv1's output
#else
                // (this build: the split-bf16 engine's conv2 in the mixed arithmetic - conv1's outputs have to stay inside the
                // e4m3 range of their q plane, 448 / 2^MIX_LG_AQ; beyond it the cross terms saturate and the product falls back
                // towards half precision: the engine would keep decoding, below its tolerance)
                (void)A2;
                (void)B2;
                const double c1 = 448.0 / std::ldexp(1.0, MIX_LG_AQ);
#endif
                lim = (float)std::max(0.0, A1 > 0 ? (c1 - B1) / A1 : 3e38);
            }
            std::memcpy(&pk.host[at], &lim, 4);
        }
        m->op16_feat_limit = pk.view<const float>(at);
    }
    // linear_out: column c*F2+f of the reference (embedding.py:118) -> column f*C+c (the conv2 GEMM's natural output)
    if (!lm) {
        std::vector<int> perm((size_t)(C * F2));
        for (int64_t f = 0; f < F2; ++f)
            for (int64_t ch = 0; ch < C; ++ch) perm[(size_t)(f * C + ch)] = (int)(ch * F2 + f);
        m->linear_out = pk.linear({"src_embed.linear_out"}, d, C * F2, &perm);
        if (m->fp8_enc && (m->fp8_scope & CN_FP8_LINEAR) && m->conv2_f8w && linear256_f8_applies((int)d, (int)(C * F2))) {  // config 5: linear_out on e4m3 operands as well
            const size_t fat = pk.reserve((size_t)d * C * F2), qat = pk.reserve(16);
            if (pk.fill) {
                const HostTensor* t = pk.find("src_embed.linear_out.weight", {d, C * F2});
                if (t) {
                    float mx = 0.f;
                    for (float v : t->data) mx = std::max(mx, std::fabs(v));
                    const int lg = cn_e4m3_exp(mx);
                    const float scale = std::ldexp(1.f, lg);
                    for (int64_t r = 0; r < d; ++r)
                        for (int64_t cc = 0; cc < C * F2; ++cc)
                            pk.host[fat + (size_t)(r * C * F2 + cc)] = cn_f32_to_e4m3_host(t->data[r * C * F2 + perm[(size_t)cc]] * scale);
                    const int q[4] = {127 - lg, 127 - (int)std::lround(std::log2(FP8_S_IMG)), 0, 0};
                    std::memcpy(&pk.host[qat], q, 16);
                }
            }
            m->linear_f8w = pk.view<void>(fat);
            m->linear_f8q = pk.view<int>(qat);
        }
    }
    auto self_layer = [&](const std::string& p, const std::string& att, int64_t dff, int nnorm, bool ff_swish = false) {
        Layer L;
        L.has_self = true;
        L.ff_swish = ff_swish;
        L.qkv = pk.linear({p + "." + att + ".linears.0", p + "." + att + ".linears.1", p + "." + att + ".linears.2"}, d, d);
        L.self_o = pk.linear({p + "." + att + ".linears.3"}, d, d);
        pk.ffn(L, p, dff, d);
        for (int i = 0; i < nnorm; ++i) L.n[i] = pk.norm(p + ".sublayer." + std::to_string(i) + ".norm", d);
        return L;
    };
    auto add_src = [&](Layer& L, const std::string& p) {
        L.has_src = true;
        L.src_q = pk.linear({p + ".src_attn.linears.0"}, d, d);
        L.src_kv = pk.linear({p + ".src_attn.linears.1", p + ".src_attn.linears.2"}, d, d);
        L.src_o = pk.linear({p + ".src_attn.linears.3"}, d, d);
    };
    m->enc.clear();
    m->extra.clear();
    m->sad.clear();
    m->mad.clear();
    const int64_t H = c.n_head;
    for (int n = 0; n < c.n_enc; ++n) {
        const std::string p = "encoder.layers." + std::to_string(n);
        if (c.conf_enc)
            m->enc.push_back(pk.conformer_layer(p, "src_embed.pos_enc.embedding.weight", c.d_encff, c.enc_kernel, c.enc_max_rel, d, H, 4));
        else {
            Layer L = self_layer(p, "self_attn", c.d_encff, 2);
            if (m->fp8_enc) {  // config 5: e4m3fn copies of the four products of an encoder layer
                pk.quant8(L.qkv, {p + ".self_attn.linears.0", p + ".self_attn.linears.1", p + ".self_attn.linears.2"}, d);
                pk.quant8(L.self_o, {p + ".self_attn.linears.3"}, d);
                pk.quant8(L.w1, {p + ".feed_forward.w_1"}, c.d_encff);
                pk.quant8(L.w2, {p + ".feed_forward.w_2"}, d);
            }
            m->enc.push_back(L);
        }
    }
    m->enc_norm = pk.norm("encoder.norm", d);
    // conformer layer = row-chain launches around the attention and the depthwise-convolution kernels:
    //   A: x += 0.5 FFN1(LN x);            next: self-attention pre-norm + Q|K|V
    //   B: x += W_o ctx;                   next: convolution pre-norm + pointwise conv 1 (2d columns)
    //   C: x += pointwise conv 2 (module); self layers: x += 0.5 FFN2(LN x) (+ `final_norm` -> output after the last one)
    //      mixed-attention layers: next: source-attention pre-norm + its query projection, then
    //   D: x += W_o' ctx;  x += 0.5 FFN2(LN x) (+ `final_norm`)
    auto conf_layer_chains = [&](Layer& L, const std::string& p, int64_t dff, bool mixed, const std::string& final_norm) {
        Packer::ChainSpec a, b, cc, dd;
        a.ln1 = p + ".sublayer.0.norm";
        a.ffn = p + ".feed_forward1";
        a.dff = dff;
        a.ffn_scale = 0.5f;
        a.swish = true;
        a.nln = p + ".sublayer.2.norm";
        a.tails = {p + ".self_attn.linears.0", p + ".self_attn.linears.1", p + ".self_attn.linears.2"};
        a.tail_rows = d;
        L.cf_a = pk.chain_stream(a, d);
        b.wo = p + ".self_attn.linears.3";
        b.nln = p + ".sublayer.1.norm";
        b.tails = {p + ".conv_module.pointwise_conv1"};
        b.tail_rows = 2 * d;
        b.tail_conv = true;
        L.cf_b = pk.chain_stream(b, d);
        cc.wo = p + ".conv_module.pointwise_conv2";
        cc.wo_conv = true;
        if (!mixed) {
            cc.ln1 = p + ".sublayer.3.norm";
            cc.ffn = p + ".feed_forward2";
            cc.dff = dff;
            cc.ffn_scale = 0.5f;
            cc.swish = true;
            cc.nln = final_norm;
        } else {
            cc.nln = p + ".sublayer.3.norm";
            cc.tails = {p + ".src_attn.linears.0"};
            cc.tail_rows = d;
            dd.wo = p + ".src_attn.linears.3";
            dd.ln1 = p + ".sublayer.4.norm";
            dd.ffn = p + ".feed_forward2";
            dd.dff = dff;
            dd.ffn_scale = 0.5f;
            dd.swish = true;
            dd.nln = final_norm;
            L.cf_d = pk.chain_stream(dd, d);
        }
        L.cf_c = pk.chain_stream(cc, d);
    };
    if (c.conf_enc && pk.chain_ok(d, c.d_encff) && c.d_encff % 128 == 0)
        for (int n = 0; n < c.n_enc; ++n)
            conf_layer_chains(m->enc[n], "encoder.layers." + std::to_string(n), c.d_encff, false,
                              n + 1 == c.n_enc ? "encoder.norm" : "");
    m->enc_chain.clear();
    m->kv_cols = 0;
    // fp8 engine: the same chains with the feed-forward units in e4m3 (chain.hip, F8 form) when d_ff allows, else the unfused
    // per-product path (run_enc_layer_fp8)
    static const bool f8_unfused = cn_exp_env("CASSNAT_FP8_UNFUSED") != nullptr;
    const bool f8c = m->fp8_enc && !lm && !f8_unfused && c.d_encff % 256 == 0;
    // CASSNAT_FP8_LAYERS: bit n set = layer n's feed-forward products in e4m3 (accuracy experiments: tools/fp8_accuracy.py)
    static const unsigned f8_layers = cn_exp_env("CASSNAT_FP8_LAYERS") ? (unsigned)strtoul(cn_exp_env("CASSNAT_FP8_LAYERS"), nullptr, 0) : ~0u;
    auto f8_at = [&](int n) {
        return f8c && (m->fp8_scope & CN_FP8_FFN) && n >= c.fp8_ffn_first_layer && ((f8_layers >> (n & 31)) & 1u);
    };
    if (!c.conf_enc && (!m->fp8_enc || f8c) && pk.chain_ok(d, c.d_encff))  // (the TransformerLM's layers are encoder layers: same chains)
        for (int n = 0; n < c.n_enc; ++n) {
            const std::string p = "encoder.layers." + std::to_string(n), q = "encoder.layers." + std::to_string(n + 1);
            if (n + 1 < c.n_enc)
                m->enc_chain.push_back(pk.chain(p + ".self_attn.linears.3", p + ".sublayer.1.norm", p, c.d_encff,
                                                q + ".sublayer.0.norm",
                                                {q + ".self_attn.linears.0", q + ".self_attn.linears.1", q + ".self_attn.linears.2"}, d, f8_at(n)));
            else {
                // the last launch also projects enc_h = encoder.norm(x) onto the cross-attention K|V of every decoder-side
                // layer (extractor, then mixed-attention decoder): three 8000-row GEMM launches per batch become the tail of
                // a launch that already holds enc_h in registers
                std::vector<std::string> kv_tails;
                if (!lm && !c.ast && !c.conf_dec && pk.chain_ok(d, c.d_decff) && (c.n_extra + c.n_mix_dec) * 2 * d <= 1536) {
                    for (int j = 0; j < c.n_extra; ++j)
                        for (int w = 1; w <= 2; ++w)
                            kv_tails.push_back("acembed_extractor.layers." + std::to_string(j) + ".src_attn.linears." + std::to_string(w));
                    for (int j = 0; j < c.n_mix_dec; ++j)
                        for (int w = 1; w <= 2; ++w)
                            kv_tails.push_back("decoder.layers." + std::to_string(j) + ".src_attn.linears." + std::to_string(w));
                }
                m->kv_cols = (int)kv_tails.size() * (int)d;
                m->enc_chain.push_back(
                    pk.chain(p + ".self_attn.linears.3", p + ".sublayer.1.norm", p, c.d_encff, "encoder.norm", kv_tails, d, f8_at(n)));
            }
        }
    m->enc_entry = ChainRef();
    if (!m->enc_chain.empty())
        m->enc_entry = pk.chain("", "", "", 0, "encoder.layers.0.sublayer.0.norm",
                                {"encoder.layers.0.self_attn.linears.0", "encoder.layers.0.self_attn.linears.1",
                                 "encoder.layers.0.self_attn.linears.2"}, d);
    const std::string dec_table = "acembed_extractor.layers.0.pos_enc.embedding.weight";
    for (int n = 0; n < c.n_extra; ++n) {
        const std::string p = "acembed_extractor.layers." + std::to_string(n);
        Layer L;
        add_src(L, p);
        if (c.conf_dec) {  // SrcAttLayer (fanat_conformer_blocks.py:41-60): one norm, Swish FFN of width d_ff
            L.conformer = true;
            pk.ffn_plain(L.w1, L.w2, p + ".feed_forward", c.d_ff, d);
            L.n[0] = pk.norm(p + ".sublayer.norm", d);
        } else {
            pk.ffn(L, p, c.d_decff, d);
            L.n[0] = pk.norm(p + ".sublayer.0.norm", d);
            L.n[1] = pk.norm(p + ".sublayer.1.norm", d);
        }
        m->extra.push_back(L);
    }
    for (int n = 0; n < c.n_self_dec; ++n) {
        const std::string p = "embed_mapper.layers." + std::to_string(n);
        if (c.conf_dec)
            m->sad.push_back(pk.conformer_layer(p, dec_table, c.d_decff, c.dec_kernel, c.dec_max_rel, d, H, 4));
        else
            m->sad.push_back(self_layer(p, "self_attn", c.d_decff, 2));
    }
    for (int n = 0; n < c.n_mix_dec; ++n) {
        const std::string p = "decoder.layers." + std::to_string(n);
        if (c.conf_dec) {
            Layer L = pk.conformer_layer(p, dec_table, c.d_decff, c.dec_kernel, c.dec_max_rel, d, H, 5);
            add_src(L, p);
            m->mad.push_back(L);
        } else {
            // (cfg.ast == 1 with conf_enc: the reference's models/conformer.py - transformer decoder layers with Swish FFNs)
            Layer L = self_layer(p, "self_attn", c.d_decff, 3, c.ast == 1 && c.conf_enc);
            add_src(L, p);
            m->mad.push_back(L);
        }
    }
    if (c.conf_dec && pk.chain_ok(d, c.d_decff) && c.d_decff % 128 == 0) {
        for (int n = 0; n < c.n_self_dec; ++n)
            conf_layer_chains(m->sad[n], "embed_mapper.layers." + std::to_string(n), c.d_decff, false,
                              (c.n_mix_dec == 0 && n + 1 == c.n_self_dec) ? "decoder.norm" : "");
        for (int n = 0; n < c.n_mix_dec; ++n)
            conf_layer_chains(m->mad[n], "decoder.layers." + std::to_string(n), c.d_decff, true,
                              n + 1 == c.n_mix_dec ? "decoder.norm" : "");
    }
    if (m->kv_cols > 0) {
        for (size_t j = 0; j < m->extra.size(); ++j) m->extra[j].kv_slot = (int)j;
        for (size_t j = 0; j < m->mad.size(); ++j) m->mad[j].kv_slot = (int)(m->extra.size() + j);
    }
    if (!lm) m->dec_norm = pk.norm("decoder.norm", d);
    // decoder-side sublayers of the NAT model in execution order, each with the chain that follows its attention
    m->dec_steps.clear();
    if (!c.ast && !c.conf_dec && pk.chain_ok(d, c.d_decff)) {
        struct Sub {
            int stack, layer;
            bool self, ffn;
            std::string p, att, pre, ffn_norm;  // layer prefix, attention module, its pre-norm, the FFN's pre-norm
        };
        std::vector<Sub> subs;
        for (int n = 0; n < c.n_extra; ++n) {
            const std::string p = "acembed_extractor.layers." + std::to_string(n);
            subs.push_back({0, n, false, true, p, p + ".src_attn", p + ".sublayer.0.norm", p + ".sublayer.1.norm"});
        }
        for (int n = 0; n < c.n_self_dec; ++n) {
            const std::string p = "embed_mapper.layers." + std::to_string(n);
            subs.push_back({1, n, true, true, p, p + ".self_attn", p + ".sublayer.0.norm", p + ".sublayer.1.norm"});
        }
        for (int n = 0; n < c.n_mix_dec; ++n) {
            const std::string p = "decoder.layers." + std::to_string(n);
            subs.push_back({2, n, true, false, p, p + ".self_attn", p + ".sublayer.0.norm", ""});
            subs.push_back({2, n, false, true, p, p + ".src_attn", p + ".sublayer.1.norm", p + ".sublayer.2.norm"});
        }
        auto in_proj = [&](const Sub& u) -> std::vector<std::string> {
            if (u.self) return {u.att + ".linears.0", u.att + ".linears.1", u.att + ".linears.2"};
            return {u.att + ".linears.0"};
        };
        for (size_t k = 0; k < subs.size(); ++k) {
            const Sub& u = subs[k];
            DecStep st;
            st.stack = u.stack;
            st.layer = u.layer;
            st.self = u.self;
            const bool final = k + 1 == subs.size();
            st.chain = pk.chain(u.att + ".linears.3", u.ffn_norm, u.p, u.ffn ? c.d_decff : 0,
                                final ? std::string("decoder.norm") : subs[k + 1].pre,
                                final ? std::vector<std::string>{} : in_proj(subs[k + 1]), d);
            if (k == 0 || (u.stack == 2 && u.layer == 0 && u.self)) st.entry = pk.chain("", "", "", 0, u.pre, in_proj(u), d);
            m->dec_steps.push_back(st);
        }
    }
    if (c.ast) {
        const size_t at = pk.reserve((size_t)V * d * 4);
        if (pk.fill) {
            const HostTensor* t = pk.find(lm ? "text_embed.0.lut.weight" : "tgt_embed.0.lut.weight", {V, d});
            if (t) std::memcpy(&pk.host[at], t->data.data(), (size_t)V * d * 4);
        }
        m->tgt_lut = pk.view<float>(at);
    } else {
        m->tgt_lut = nullptr;
    }
    if (!lm) m->ctc_gen = pk.generator("ctc_generator.proj", V, d);
    m->att_gen = pk.generator(lm ? "out_generator.proj" : "att_generator.proj", V, d);
    {
        const size_t at = pk.reserve((size_t)m->pe_rows * d * 4);
        if (pk.fill) std::memcpy(&pk.host[at], m->pe_host.data(), (size_t)m->pe_rows * d * 4);
        m->pe = pk.view<float>(at);
    }
}

}  // namespace

// Two passes of pack_model.  The first has no blob yet: it builds the staging image (when this handle holds the tensors) and
// learns the size.  With the blob allocated, borrowed or kept, the second - layout only - makes every view the handle keeps,
// as blob + offset, and leaves the handle's other packing state (Layer flags, kv_cols, dec_steps).  So nothing but staging
// bytes may depend on Packer::fill: both passes must reserve, and set, the same things.
int build_weights(cn_model* m) {
    Packer pk(m, !m->host.empty() && !m->blob_borrowed, nullptr);
    pack_model(m, pk);
    if (!pk.missing.empty()) {
        cn_set_error("cn_model_finalize: missing or mis-shaped parameters: " + pk.missing);
        return -1;
    }
    if (m->blob_borrowed) {
        if (m->blob_bytes != pk.off) {
            cn_set_error("cn_model_create_shared: the donor's weight blob has another layout (" + std::to_string(m->blob_bytes) +
                         " vs " + std::to_string(pk.off) + " bytes): the model hyper-parameters must agree");
            return -1;
        }
    } else {
        if (m->blob && (m->blob_bytes != pk.off || m->blob_owner.use_count() > 1)) {  // (a blob others still use is left to them)
            m->blob_owner.reset();
            m->blob = nullptr;
        }
        if (!m->blob) {
            auto owner = std::make_shared<cn_model::BlobOwner>();
            CN_HIP_CHECK(hipMalloc((void**)&owner->p, pk.off));
            m->blob_owner = owner;
            m->blob = owner->p;
        }
        m->blob_bytes = pk.off;
        if (pk.fill) CN_HIP_CHECK(hipMemcpy(m->blob, pk.host.data(), pk.off, hipMemcpyHostToDevice));
    }
    Packer views(m, false, m->blob);
    pack_model(m, views);
    if (views.off != pk.off) {
        cn_set_error("cn_model_finalize: the two passes over the weight layout disagree (" + std::to_string(pk.off) + " vs " +
                     std::to_string(views.off) + " bytes)");
        return -1;
    }
    return 0;
}

}  // namespace cn_host
