// The scoring core of the ARPA n-gram model (include/cassnat_hip.h has the contract and the hashing): hash probes, the per-word score
// - serial, and as independent probes for a group of threads - and the piece monoid, written once as __host__ __device__ code; and
// the validity check of a cn_ngram_desc.  ngram.hip (the ESA ranker), the CTC prefix beam search (ctc_ngram_search.h) and the AST beam
// search (ast_ngram_search.h) are built from it; a plain C++ compiler reads it too (tools/*_check.cpp).
#pragma once
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/cassnat_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define NG_HD __host__ __device__ __forceinline__
#else
#define NG_HD inline
#endif

constexpr uint64_t NG_P = 0x9E3779B97F4A7C15ull;       // = 5 mod 8: P^n = 1 mod 2^64 only for n = 0 mod 2^62, so P^len = 1 <=> empty
constexpr uint64_t NG_SEED = 0x243F6A8885A308D3ull;
constexpr uint64_t NG_FOREIGN = 0xD1B54A32D192ED03ull;  // what an id outside the vocabulary hashes to
constexpr int NG_MAX_ORDER = 8;
constexpr int NG_HIST = NG_MAX_ORDER - 1;
constexpr float NG_UNK_LOGPROB = -100.0f;  // kenlm's default unknown_missing_logprob

struct NgPiece {
    uint64_t h, pw;
    int starts;
};

NG_HD uint64_t ng_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// n-gram keys fold the ids from the LAST word to the first, so that the k-grams that end in one word, k = 1, 2, .., share their work
NG_HD uint64_t ng_fold(uint64_t k, int32_t id) {
    k = (k ^ (uint64_t)(uint32_t)(id + 1)) * 0xFF51AFD7ED558CCDull;
    return k ^ (k >> 32);
}

NG_HD uint64_t ng_gram_key(uint64_t folded, int n, uint64_t mask) { return ng_mix(folded + (uint64_t)n * 0xC4CEB9FE1A85EC53ull) & mask; }

NG_HD NgPiece ng_combine(const NgPiece& a, const NgPiece& b) {
    if (b.starts) return b;
    NgPiece r;
    r.h = a.h * b.pw + b.h;
    r.pw = a.pw * b.pw;
    r.starts = a.starts;
    return r;
}

NG_HD NgPiece ng_piece(const cn_ngram_desc& d, int32_t t, bool real) {
    NgPiece r;
    if (!real) {
        r.h = 0, r.pw = 1, r.starts = 0;
    } else if (t < 0 || t >= d.vocab) {
        r.h = NG_FOREIGN, r.pw = NG_P, r.starts = 1;
    } else {
        r.h = d.piece_hash[t], r.pw = d.piece_pow[t], r.starts = d.piece_starts[t] != 0;
    }
    return r;
}

NG_HD int32_t ng_word_id(const cn_ngram_desc& d, uint64_t h) {
    const uint64_t key = h & d.key_mask, m = (uint64_t)d.word_slots - 1;
    uint64_t s = ng_mix(key) & m;
    for (int64_t n = 0; n < d.word_slots; ++n, s = (s + 1) & m) {  // (a table is at most half full: an empty slot ends the walk)
        if (d.word_ids[s] < 0) break;
        if (d.word_keys[s] == key) return d.word_ids[s];
    }
    return d.unk;
}

NG_HD bool ng_gram(const cn_ngram_desc& d, uint64_t key, float* prob, float* bo) {
    const uint64_t m = (uint64_t)d.gram_slots - 1;
    uint64_t s = key & m;
    for (int64_t n = 0; n < d.gram_slots; ++n, s = (s + 1) & m) {
        const float p = d.gram_prob[s];
        if (p == std::numeric_limits<float>::infinity()) break;
        if (d.gram_keys[s] == key) {
            *prob = p;
            *bo = d.gram_bo[s];
            return true;
        }
    }
    return false;
}

// h[-1] is the word before w, h[-c] the oldest word of its history
NG_HD float ng_word_score(const cn_ngram_desc& d, const int32_t* h, int c, int32_t w) {
    uint64_t keys[NG_MAX_ORDER];  // keys[k - 1]: the k-gram that ends in w
    uint64_t f = ng_fold(NG_SEED, w);
    keys[0] = ng_gram_key(f, 1, d.key_mask);
#pragma unroll
    for (int i = 1; i < NG_MAX_ORDER; ++i) {
        if (i <= c) {
            f = ng_fold(f, h[-i]);
            keys[i] = ng_gram_key(f, i + 1, d.key_mask);
        }
    }
    int k = 0;
    float s = NG_UNK_LOGPROB, bo = 0.f;  // (every id of a model has its 1-gram: the default is what a damaged table gives)
#pragma unroll
    for (int i = NG_MAX_ORDER; i >= 1; --i) {
        if (k == 0 && i <= c + 1 && ng_gram(d, keys[i - 1], &s, &bo)) k = i;
    }
    if (k == 0) k = 1;
    uint64_t g = NG_SEED;
#pragma unroll
    for (int j = 1; j < NG_MAX_ORDER; ++j) {
        if (j <= c) {
            g = ng_fold(g, h[-j]);
            float p;
            if (j >= k && ng_gram(d, ng_gram_key(g, j, d.key_mask), &p, &bo)) s += bo;
        }
    }
    return s;
}

// ---- the same score from independent table probes ---------------------------------------------------------------------------------
constexpr int NG_TASKS = 2 * NG_MAX_ORDER;  // probes of one word: NG_MAX_ORDER k-grams, NG_MAX_ORDER - 1 back-off weights, one idle
struct NgProbe {
    float prob, bo;
    int found;
};

// The table probes of ng_word_score(d, h, c, w), one per task, independent of each other: task i < NG_MAX_ORDER is the (i + 1)-gram
// that ends in w (needs i <= c), task NG_MAX_ORDER + j - 1 the back-off weight of the j-gram h[-j .. -1] (1 <= j <= c).
NG_HD void ng_probe(const cn_ngram_desc& d, const int32_t* h, int c, int32_t w, int task, NgProbe* out) {
    out->prob = 0.f, out->bo = 0.f, out->found = 0;
    const bool gram = task < NG_MAX_ORDER;
    const int n = gram ? task : task - NG_MAX_ORDER + 1;  // history ids folded
    if (n > c || (!gram && n < 1) || n >= NG_MAX_ORDER) return;
    uint64_t f = gram ? ng_fold(NG_SEED, w) : NG_SEED;
    for (int i = 1; i <= n; ++i) f = ng_fold(f, h[-i]);
    out->found = ng_gram(d, ng_gram_key(f, gram ? n + 1 : n, d.key_mask), &out->prob, &out->bo) ? 1 : 0;
}

// ng_word_score's float32 sum from the probes: the longest k-gram's probability, then the back-off weights for j = k .. c
NG_HD float ng_probe_score(const NgProbe* pr, int c) {
    int k = 0;
    float s = NG_UNK_LOGPROB;
    for (int i = NG_MAX_ORDER; i >= 1; --i) {
        if (k == 0 && i <= c + 1 && pr[i - 1].found) k = i, s = pr[i - 1].prob;
    }
    if (k == 0) k = 1;
    for (int j = 1; j < NG_MAX_ORDER; ++j) {
        if (j <= c && j >= k && pr[NG_MAX_ORDER + j - 1].found) s += pr[NG_MAX_ORDER + j - 1].bo;
    }
    return s;
}

// ---- host only -------------------------------------------------------------------------------------------------------------------
// "" when the desc can be scored with (pointers of the caller's side: not dereferenced here), else what is wrong
inline std::string ng_check_desc(const cn_ngram_desc& d) {
    if (!d.word_keys || !d.word_ids || !d.gram_keys || !d.gram_prob || !d.gram_bo || !d.piece_hash || !d.piece_pow || !d.piece_starts)
        return "null table in the desc";
    if (d.order < 1 || d.order > NG_MAX_ORDER) return "order " + std::to_string(d.order) + " is outside 1 .. 8";
    if (d.word_slots < 1 || (d.word_slots & (d.word_slots - 1)) || d.gram_slots < 1 || (d.gram_slots & (d.gram_slots - 1)))
        return "the slot counts must be powers of two";
    if (d.vocab < 0) return "vocab must not be negative";
    return "";
}
