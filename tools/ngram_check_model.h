// The in-memory n-gram model of the stand-alone host checks (tools/ctc_ngram_check.cpp, tools/ast_ngram_check.cpp): dyadic values,
// tables on the heap of exactly their slot counts, a small vocabulary of pieces; and the checks' failure counter.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "ctc_ngram_search.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
        }                                     \
    } while (0)

uint64_t hash_bytes(const std::string& s, uint64_t* pw) {
    uint64_t h = 0, p = 1;
    for (unsigned char c : s) h = h * NG_P + ((uint64_t)c + 1), p *= NG_P;
    *pw = p;
    return h;
}

// tables of one model over the heap, each of exactly its slot count
struct Model {
    std::unique_ptr<uint64_t[]> word_keys, gram_keys, piece_hash, piece_pow;
    std::unique_ptr<int32_t[]> word_ids;
    std::unique_ptr<float[]> gram_prob, gram_bo;
    std::unique_ptr<uint8_t[]> piece_starts;
    cn_ngram_desc d;

    void add_word(uint64_t h, int32_t id) {
        const uint64_t key = h & d.key_mask, m = (uint64_t)d.word_slots - 1;
        uint64_t s = ng_mix(key) & m;
        while (word_ids[s] >= 0) s = (s + 1) & m;
        word_keys[s] = key, word_ids[s] = id;
    }
    bool add_gram(const int32_t* ids, int n, float prob, float bo) {
        uint64_t f = NG_SEED;
        for (int i = n - 1; i >= 0; --i) f = ng_fold(f, ids[i]);
        const uint64_t key = ng_gram_key(f, n, d.key_mask), m = (uint64_t)d.gram_slots - 1;
        uint64_t s = key & m;
        for (; gram_prob[s] != std::numeric_limits<float>::infinity(); s = (s + 1) & m)
            if (gram_keys[s] == key) return false;
        gram_keys[s] = key, gram_prob[s] = prob, gram_bo[s] = bo;
        return true;
    }
};

// words: <unk> <s> </s> then `words`; pieces: 4 specials (no separator), "_w" for every word, continuations, a bare separator
std::unique_ptr<Model> make_model(int order, std::mt19937& rng, const std::vector<std::string>& words, std::vector<std::string>* pieces,
                                  std::vector<uint8_t>* starts) {
    auto m = std::make_unique<Model>();
    const int n_ids = (int)words.size() + 3;
    int64_t ws = 2, gs = 2;
    while (ws < 2 * (n_ids + 1)) ws *= 2;
    const int per_order = 40;
    while (gs < 2 * (n_ids + per_order * (order - 1) + 1)) gs *= 2;
    memset(&m->d, 0, sizeof(m->d));
    m->word_keys.reset(new uint64_t[ws]()), m->word_ids.reset(new int32_t[ws]);
    m->gram_keys.reset(new uint64_t[gs]()), m->gram_prob.reset(new float[gs]), m->gram_bo.reset(new float[gs]());
    for (int64_t i = 0; i < ws; ++i) m->word_ids[i] = -1;
    for (int64_t i = 0; i < gs; ++i) m->gram_prob[i] = std::numeric_limits<float>::infinity();
    m->d.word_slots = ws, m->d.gram_slots = gs, m->d.key_mask = ~0ull, m->d.order = order;
    m->d.unk = 0, m->d.bos = 1, m->d.eos = 2;
    auto dyadic = [&](int lo) { return -(float)(lo + (int)(rng() % (257 - lo))) / 64.f; };
    uint64_t pw;
    for (int id = 0; id < n_ids; ++id) {
        const std::string w = id == 0 ? "<unk>" : id == 1 ? "<s>" : id == 2 ? "</s>" : words[id - 3];
        m->add_word(hash_bytes(w, &pw), id);
        m->add_gram(&id, 1, id == 1 ? -99.f : dyadic(1), id == 2 ? 0.f : dyadic(0));
    }
    for (int k = 2; k <= order; ++k)
        for (int i = 0; i < per_order; ++i) {
            int32_t ids[NG_MAX_ORDER];
            for (int j = 0; j < k; ++j) ids[j] = j == 0 && rng() % 4 == 0 ? 1 : 3 + (int)(rng() % words.size());
            if (rng() % 5 == 0) ids[k - 1] = 2;
            m->add_gram(ids, k, dyadic(1), k < order ? dyadic(0) : 0.f);
        }
    pieces->assign({"blank", "sos", "eos", "unk"});
    starts->assign(4, 0);
    for (const std::string& w : words) pieces->push_back(w), starts->push_back(1);
    for (const char* c : {"a", "b", "c", "bc"}) pieces->push_back(c), starts->push_back(0);
    pieces->push_back(""), starts->push_back(1);
    const int V = (int)pieces->size();
    m->piece_hash.reset(new uint64_t[V]), m->piece_pow.reset(new uint64_t[V]), m->piece_starts.reset(new uint8_t[V]);
    for (int i = 0; i < V; ++i) m->piece_hash[i] = hash_bytes((*pieces)[i], &m->piece_pow[i]), m->piece_starts[i] = (*starts)[i];
    m->d.word_keys = m->word_keys.get(), m->d.word_ids = m->word_ids.get(), m->d.gram_keys = m->gram_keys.get();
    m->d.gram_prob = m->gram_prob.get(), m->d.gram_bo = m->gram_bo.get();
    m->d.piece_hash = m->piece_hash.get(), m->d.piece_pow = m->piece_pow.get(), m->d.piece_starts = m->piece_starts.get();
    m->d.vocab = V;
    return m;
}

}  // namespace
