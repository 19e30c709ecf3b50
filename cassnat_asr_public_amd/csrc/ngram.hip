// ARPA n-gram model: the ESA ranker `rank_model: n-gram` (src/models/cassnat.py:522-535 scores every sample's text with kenlm on
// the host; here the samples' token rows are scored where they are).  See include/cassnat_hip.h for the contract and the hashing.
//
// One scoring core, written once as __host__ __device__ code (hash probes, the per-word score, the piece monoid: ngram_core.h), under
// two entry points: cn_ngram_score_host walks a row piece by piece, cn_op_ngram_score gives a row to one wave:
//   * lanes take the row's tokens 64 at a time and load their piece's (H, P^len, starts) triple; a dropped token or a position behind
//     the row's length is the monoid's identity (0, 1, no);
//   * a segmented inclusive scan over combine(a, b) = b.starts ? b : (a.h * b.pw + b.h, a.pw * b.pw, a.starts) - six shuffle steps -
//     and the carry of the chunks before give every lane the word spelled up to and including its piece; a word may span chunks;
//   * a word ends where the next piece begins with a separator: the lane of THAT piece holds the finished word in its exclusive scan
//     value and probes the word table for it (an empty word - P^len = 1 - does not exist); the row's last word is in the final carry;
//   * the ids are compacted in order into LDS (ballot + prefix count) behind the last order - 1 ids of the chunks before;
//   * lanes over words score independently from the LDS ids; the word scores are added in word order, float32.
// Nothing here is sized by the row: stride is bounded by int32 alone.  The kernel waits on table look-ups (a handful of dependent
// loads per word); there is no matrix work in it.  The ARPA reader (cn_ngram_counts / cn_ngram_parse) is host code in this file too:
// it fills the very tables the core probes, with the core's own hash functions.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/cassnat_hip.h"
#include "kernels.h"
#include "ngram_core.h"

// ---- host scorer ---------------------------------------------------------------------------------------------------------------
static float ng_score_row_host(const cn_ngram_desc& d, const int32_t* tok, int n, int32_t drop_id) {
    int32_t ids[NG_HIST + 1];  // the last NG_HIST ids, then the word being scored
    for (int i = 0; i < NG_HIST; ++i) ids[i] = d.bos;
    int before = 0;
    float acc = 0.f;
    auto word = [&](int32_t w) {
        const int c = before + 1 < d.order - 1 ? before + 1 : d.order - 1;
        ids[NG_HIST] = w;
        acc += ng_word_score(d, ids + NG_HIST, c, w);
        for (int i = 0; i < NG_HIST; ++i) ids[i] = ids[i + 1];
        ++before;
    };
    NgPiece carry = ng_piece(d, 0, false);
    for (int i = 0; i < n; ++i) {
        const bool real = tok[i] != drop_id;
        const NgPiece pc = ng_piece(d, tok[i], real);
        if (real && pc.starts && carry.pw != 1) word(ng_word_id(d, carry.h));
        carry = ng_combine(carry, pc);
    }
    if (carry.pw != 1) word(ng_word_id(d, carry.h));
    word(d.eos);
    return acc;
}

// ---- device scorer -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ng_shfl_up(uint64_t v, int delta) {
    const unsigned lo = __shfl_up((unsigned)v, delta, 64), hi = __shfl_up((unsigned)(v >> 32), delta, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t ng_shfl(uint64_t v, int lane) {
    const unsigned lo = __shfl((unsigned)v, lane, 64), hi = __shfl((unsigned)(v >> 32), lane, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ NgPiece ng_shfl_up(const NgPiece& v, int delta) {
    NgPiece r;
    r.h = ng_shfl_up(v.h, delta), r.pw = ng_shfl_up(v.pw, delta), r.starts = __shfl_up(v.starts, delta, 64);
    return r;
}

__global__ __launch_bounds__(64) void ngram_score_kernel(cn_ngram_desc d, const int32_t* __restrict__ tok, int stride,
                                                         const int32_t* __restrict__ len, int32_t drop_id, float* __restrict__ score) {
    __shared__ int32_t ids[NG_HIST + 64 + 2];  // the last NG_HIST ids of the chunks before, then this chunk's words in order
    __shared__ float sc[64];
    const int row = blockIdx.x, lane = threadIdx.x;
    int n = len[row];
    n = n < 0 ? 0 : (n > stride ? stride : n);
    const int32_t* t_row = tok + (long long)row * stride;
    if (lane < NG_HIST) ids[lane] = d.bos;
    __syncthreads();
    int before = 0;   // words scored so far (uniform over the wave, as are acc and carry)
    float acc = 0.f;
    NgPiece carry = ng_piece(d, 0, false);

    // scores the m words at ids[NG_HIST ..), adds them in order and keeps the last NG_HIST ids for the next call
    auto score_words = [&](int m) {
        if (lane < m) {
            const int c = before + lane + 1 < d.order - 1 ? before + lane + 1 : d.order - 1;
            sc[lane] = ng_word_score(d, ids + NG_HIST + lane, c, ids[NG_HIST + lane]);
        }
        __syncthreads();
        for (int j = 0; j < m; ++j) acc += sc[j];
        const int32_t keep = lane < NG_HIST ? ids[m + lane] : 0;
        __syncthreads();
        if (lane < NG_HIST) ids[lane] = keep;
        before += m;
        __syncthreads();
    };

    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const int32_t t = i < n ? t_row[i] : drop_id;
        const bool real = i < n && t != drop_id;
        NgPiece v = ng_piece(d, t, real);
        const bool starts = real && v.starts;
        for (int delta = 1; delta < 64; delta <<= 1) {
            const NgPiece a = ng_shfl_up(v, delta);
            if (lane >= delta) v = ng_combine(a, v);
        }
        const NgPiece inc = ng_combine(carry, v);
        NgPiece ex = ng_shfl_up(inc, 1);
        if (lane == 0) ex = carry;
        const bool emit = starts && ex.pw != 1;  // this piece begins a word: the one before it, if there is one, is complete
        const int32_t id = emit ? ng_word_id(d, ex.h) : 0;
        const unsigned long long ball = __ballot(emit);
        if (emit) ids[NG_HIST + __popcll(ball & ((1ull << lane) - 1ull))] = id;
        carry.h = ng_shfl(inc.h, 63), carry.pw = ng_shfl(inc.pw, 63), carry.starts = __shfl(inc.starts, 63, 64);
        __syncthreads();
        score_words(__popcll(ball));
    }
    int m = 0;
    if (carry.pw != 1) {
        if (lane == 0) ids[NG_HIST] = ng_word_id(d, carry.h);
        m = 1;
    }
    if (lane == 0) ids[NG_HIST + m] = d.eos;
    ++m;
    __syncthreads();
    score_words(m);
    if (lane == 0) score[row] = acc;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
static int ng_check(const char* who, const cn_ngram_desc* d, const void* tok, int32_t stride, const void* len, int32_t rows, const void* score) {
    const std::string w(who);
    if (!d || !tok || !len || !score) {
        cn_set_error(w + ": null argument");
        return -1;
    }
    const std::string bad = rows < 1 || stride < 1 ? "rows and stride must be positive" : ng_check_desc(*d);
    if (!bad.empty()) {
        cn_set_error(w + ": " + bad);
        return -1;
    }
    return 0;
}

extern "C" int32_t cn_ngram_desc_size(void) { return (int32_t)sizeof(cn_ngram_desc); }

extern "C" int cn_ngram_score_host(const cn_ngram_desc* desc, const int32_t* tok, int32_t stride, const int32_t* len, int32_t rows,
                                   int32_t drop_id, float* score) {
    CN_TRY(ng_check("cn_ngram_score_host", desc, tok, stride, len, rows, score));
    for (int32_t r = 0; r < rows; ++r) {
        const int n = len[r] < 0 ? 0 : (len[r] > stride ? stride : len[r]);
        score[r] = ng_score_row_host(*desc, tok + (long long)r * stride, n, drop_id);
    }
    return 0;
}

extern "C" int cn_op_ngram_score(const cn_ngram_desc* desc, const int32_t* tok_dev, int32_t stride, const int32_t* len_dev, int32_t rows,
                                 int32_t drop_id, float* score_dev, void* stream) {
    CN_TRY(ng_check("cn_op_ngram_score", desc, tok_dev, stride, len_dev, rows, score_dev));
    hipLaunchKernelGGL(ngram_score_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, *desc, tok_dev, stride, len_dev, drop_id,
                       score_dev);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the ARPA reader (host) ----------------------------------------------------------------------------------------------------
namespace {
struct NgReader {
    const char *p, *end;
    long long line = 0;
    // the next line without its line end and without blanks at either side; false at the end of the text
    bool next(const char** b, const char** e) {
        if (p >= end) return false;
        const char* q = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char *lb = p, *le = q ? q : end;
        p = q ? q + 1 : end;
        ++line;
        while (lb < le && (*lb == ' ' || *lb == '\t' || *lb == '\r')) ++lb;
        while (le > lb && (le[-1] == ' ' || le[-1] == '\t' || le[-1] == '\r')) --le;
        *b = lb, *e = le;
        return true;
    }
};

int ng_fail(long long line, const std::string& what) {
    cn_set_error("ARPA file, line " + std::to_string(line) + ": " + what);
    return -1;
}

bool ng_is(const char* b, const char* e, const char* text) { return (size_t)(e - b) == strlen(text) && memcmp(b, text, (size_t)(e - b)) == 0; }

// "\k-grams:" -> k, else 0
int ng_section(const char* b, const char* e) {
    if (e - b < 9 || *b != '\\') return 0;
    int k = 0;
    const char* q = b + 1;
    while (q < e && *q >= '0' && *q <= '9' && k < 1000) k = k * 10 + (*q++ - '0');
    return q > b + 1 && ng_is(q, e, "-grams:") ? k : 0;
}

// reads the header up to and including the first line behind the `ngram k=` lines (left in *b, *e; *more false at the end of the text)
int ng_header(NgReader& rd, int64_t* counts, const char** b, const char** e, bool* more) {
    for (int k = 0; k <= NG_MAX_ORDER; ++k) counts[k] = 0;
    do {
        if (!rd.next(b, e)) return ng_fail(rd.line, "no \\data\\ line");
    } while (*b == *e);
    if (!ng_is(*b, *e, "\\data\\")) return ng_fail(rd.line, "the first line must be \\data\\");
    int order = 0;
    while ((*more = rd.next(b, e))) {
        if (*b == *e) continue;
        if (**b == '\\') break;
        if (*e - *b < 9 || memcmp(*b, "ngram ", 6) != 0) return ng_fail(rd.line, "expected `ngram k=count`");
        char* q = nullptr;
        const std::string s(*b + 6, *e);
        const long k = strtol(s.c_str(), &q, 10);
        if (q == s.c_str() || *q != '=') return ng_fail(rd.line, "expected `ngram k=count`");
        char* q2 = nullptr;
        const long long cnt = strtoll(q + 1, &q2, 10);
        if (q2 == q + 1 || *q2 != 0 || cnt < 0) return ng_fail(rd.line, "expected `ngram k=count`");
        if (k > NG_MAX_ORDER) return ng_fail(rd.line, "order " + std::to_string(k) + " is above 8");
        if (k != order + 1) return ng_fail(rd.line, "the `ngram k=` lines must count k = 1, 2, ..");
        order = (int)k;
        counts[k] = cnt;
    }
    if (order < 1) return ng_fail(rd.line, "no `ngram k=` line");
    counts[0] = order;
    return 0;
}

uint64_t ng_hash_bytes(const char* b, const char* e, uint64_t* pw) {
    uint64_t h = 0, p = 1;
    for (; b < e; ++b) h = h * NG_P + ((uint64_t)(unsigned char)*b + 1), p *= NG_P;
    if (pw) *pw = p;
    return h;
}

uint64_t ng_key_of(const int32_t* ids, int n, uint64_t mask) {
    uint64_t f = NG_SEED;
    for (int i = n - 1; i >= 0; --i) f = ng_fold(f, ids[i]);
    return ng_gram_key(f, n, mask);
}

struct NgTables {
    cn_ngram_desc d;  // (const views of the arrays below)
    uint64_t* word_keys;
    int32_t* word_ids;
    uint64_t* gram_keys;
    float *gram_prob, *gram_bo;
    bool add_word(uint64_t h, int32_t id) {
        const uint64_t key = h & d.key_mask, m = (uint64_t)d.word_slots - 1;
        uint64_t s = ng_mix(key) & m;
        for (; word_ids[s] >= 0; s = (s + 1) & m)
            if (word_keys[s] == key) return false;
        word_keys[s] = key, word_ids[s] = id;
        return true;
    }
    bool add_gram(uint64_t key, float prob, float bo) {
        const uint64_t m = (uint64_t)d.gram_slots - 1;
        uint64_t s = key & m;
        for (; gram_prob[s] != std::numeric_limits<float>::infinity(); s = (s + 1) & m)
            if (gram_keys[s] == key) return false;
        gram_keys[s] = key, gram_prob[s] = prob, gram_bo[s] = bo;
        return true;
    }
};

bool ng_float(const char* b, const char* e, float* out) {
    char buf[64];
    if (e <= b || e - b >= (long)sizeof(buf)) return false;
    memcpy(buf, b, (size_t)(e - b));
    buf[e - b] = 0;
    char* q = nullptr;
    *out = strtof(buf, &q);  // (the float32 nearest to the decimal text)
    return q == buf + (e - b) && std::isfinite(*out);
}
}  // namespace

extern "C" int cn_ngram_counts(const void* text, int64_t bytes, int64_t* counts) {
    if (!text || !counts || bytes < 0) {
        cn_set_error("cn_ngram_counts: null argument");
        return -1;
    }
    NgReader rd{(const char*)text, (const char*)text + bytes};
    const char *b, *e;
    bool more;
    return ng_header(rd, counts, &b, &e, &more);
}

extern "C" int cn_ngram_hash(const void* bytes, const int64_t* off, int32_t n, uint64_t* h, uint64_t* pw) {
    if (!bytes || !off || !h || !pw || n < 0) {
        cn_set_error("cn_ngram_hash: null argument");
        return -1;
    }
    for (int32_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) {
            cn_set_error("cn_ngram_hash: the offsets must not fall");
            return -1;
        }
        h[i] = ng_hash_bytes((const char*)bytes + off[i], (const char*)bytes + off[i + 1], pw + i);
    }
    return 0;
}

extern "C" int cn_ngram_parse(const void* text, int64_t bytes, int32_t hash_bits, uint64_t* word_keys, int32_t* word_ids, int64_t word_slots,
                              uint64_t* gram_keys, float* gram_prob, float* gram_bo, int64_t gram_slots, int64_t* info) {
    if (!text || !word_keys || !word_ids || !gram_keys || !gram_prob || !gram_bo || !info || bytes < 0) {
        cn_set_error("cn_ngram_parse: null argument");
        return -1;
    }
    if (hash_bits < 1 || hash_bits > 64) {
        cn_set_error("cn_ngram_parse: hash_bits must be in 1 .. 64");
        return -1;
    }
    NgReader rd{(const char*)text, (const char*)text + bytes};
    const char *b, *e;
    bool more;
    int64_t counts[NG_MAX_ORDER + 1];
    CN_TRY(ng_header(rd, counts, &b, &e, &more));
    const int order = (int)counts[0];
    int64_t total = 0;
    for (int k = 1; k <= order; ++k) total += counts[k];
    if (word_slots < 2 * (counts[1] + 1) || (word_slots & (word_slots - 1)) || gram_slots < 2 * (total + 1) || (gram_slots & (gram_slots - 1))) {
        cn_set_error("cn_ngram_parse: the slot counts must be powers of two, at least 2 * (1-grams + 1) and 2 * (n-grams + 1)");
        return -1;
    }
    NgTables t;
    memset(&t.d, 0, sizeof(t.d));
    t.d.word_keys = t.word_keys = word_keys, t.d.word_ids = t.word_ids = word_ids, t.d.word_slots = word_slots;
    t.d.gram_keys = t.gram_keys = gram_keys, t.d.gram_prob = t.gram_prob = gram_prob, t.d.gram_bo = t.gram_bo = gram_bo, t.d.gram_slots = gram_slots;
    t.d.key_mask = hash_bits == 64 ? ~0ull : (1ull << hash_bits) - 1ull;
    t.d.order = order, t.d.unk = -1;
    for (int64_t i = 0; i < word_slots; ++i) word_keys[i] = 0, word_ids[i] = -1;
    for (int64_t i = 0; i < gram_slots; ++i) gram_keys[i] = 0, gram_prob[i] = std::numeric_limits<float>::infinity(), gram_bo[i] = 0.f;

    std::vector<int32_t> higher;  // the ids of every entry of order >= 2, one entry behind the other (the closure count reads them)
    int32_t bos = -1, eos = -1, unk = -1, n_ids = 0;
    long long first_section_line = 0;
    bool ended = false;
    for (int k = 1; k <= order; ++k) {
        // (b, e) holds the section's header line
        if (!more || ng_section(b, e) != k) return ng_fail(rd.line, "expected \\" + std::to_string(k) + "-grams:");
        const long long head = rd.line;
        if (k == 1) first_section_line = head;
        int64_t seen = 0;
        while ((more = rd.next(&b, &e))) {
            if (b == e) continue;
            if (*b == '\\') break;
            if (++seen > counts[k]) return ng_fail(rd.line, "the " + std::to_string(k) + "-grams section holds more than its " + std::to_string(counts[k]) + " lines");
            const char* f[NG_MAX_ORDER + 3][2];
            int nf = 0;
            for (const char* q = b; q < e;) {
                while (q < e && (*q == ' ' || *q == '\t')) ++q;
                if (q >= e) break;
                const char* q0 = q;
                while (q < e && *q != ' ' && *q != '\t') ++q;
                if (nf < k + 3) f[nf][0] = q0, f[nf][1] = q;
                ++nf;
            }
            float prob, bo = 0.f;
            if (nf != k + 1 && nf != k + 2) return ng_fail(rd.line, "malformed line: a " + std::to_string(k) + "-gram has a probability, " + std::to_string(k) + " words and at most a back-off weight");
            if (!ng_float(f[0][0], f[0][1], &prob) || (nf == k + 2 && !ng_float(f[k + 1][0], f[k + 1][1], &bo)))
                return ng_fail(rd.line, "malformed line: not a finite number");
            int32_t ids[NG_MAX_ORDER];
            if (k == 1) {
                ids[0] = n_ids++;
                if (!t.add_word(ng_hash_bytes(f[1][0], f[1][1], nullptr), ids[0])) return ng_fail(rd.line, "two words with the same key (hash collision or a repeated word)");
                if (ng_is(f[1][0], f[1][1], "<s>")) bos = ids[0];
                if (ng_is(f[1][0], f[1][1], "</s>")) eos = ids[0];
                if (ng_is(f[1][0], f[1][1], "<unk>")) unk = ids[0];
            } else {
                for (int i = 0; i < k; ++i) {
                    ids[i] = ng_word_id(t.d, ng_hash_bytes(f[1 + i][0], f[1 + i][1], nullptr));
                    if (ids[i] < 0) return ng_fail(rd.line, "malformed line: a word that is not among the 1-grams");
                    higher.push_back(ids[i]);
                }
            }
            if (!t.add_gram(ng_key_of(ids, k, t.d.key_mask), prob, bo)) return ng_fail(rd.line, "two n-grams with the same key (hash collision or a repeated n-gram)");
        }
        if (seen != counts[k]) return ng_fail(head, "the " + std::to_string(k) + "-grams section holds " + std::to_string(seen) + " lines, its `ngram " + std::to_string(k) + "=` line says " + std::to_string(counts[k]));
    }
    ended = more && ng_is(b, e, "\\end\\");
    if (!ended) return ng_fail(rd.line, "expected \\end\\");
    if (bos < 0 || eos < 0) return ng_fail(first_section_line, std::string("the 1-grams hold no ") + (bos < 0 ? "<s>" : "</s>"));
    const int has_unk = unk >= 0;
    if (!has_unk) {  // kenlm's default for a model without <unk>
        unk = n_ids++;
        ++total;
        t.add_gram(ng_key_of(&unk, 1, t.d.key_mask), NG_UNK_LOGPROB, 0.f);
    }
    // closure: an entry whose prefix or suffix (n - 1)-gram the file does not hold (there an incremental matcher and the
    // longest-match rule can disagree)
    int64_t unclosed = 0;
    size_t at = 0;
    for (int k = 2; k <= order; ++k)
        for (int64_t i = 0; i < counts[k]; ++i, at += (size_t)k) {
            float p, w;
            const int32_t* ids = higher.data() + at;
            if (!ng_gram(t.d, ng_key_of(ids, k - 1, t.d.key_mask), &p, &w) || !ng_gram(t.d, ng_key_of(ids + 1, k - 1, t.d.key_mask), &p, &w)) ++unclosed;
        }
    info[0] = order, info[1] = n_ids, info[2] = total, info[3] = unclosed, info[4] = bos, info[5] = eos, info[6] = unk, info[7] = has_unk;
    return 0;
}
