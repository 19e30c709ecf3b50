// Stand-alone host check of the AST beam search's word n-gram fusion: the step functions the library's host entry and its kernel are
// built from (csrc/ast_ngram_search.h) run on the CPU, on a small n-gram model made in memory (ngram_check_model.h) and on crafted and
// random token rows, every array a heap block of exactly the size the functions were told.  Checked:
//   * adds = (a_word, a_eos) of a row, put together from the 2 x 15 independent probes, has the bits of a serial walk that scores
//     with ng_word_score (the scoring core) directly;
//   * the terms of a hypothesis' tokens, each given the tokens before it, plus a_eos at its end sum to the ranker's score of the row
//     (dyadic model values: exactly);
//   * ids equal to eos and ids outside [0, vocab) change nothing; the desc check refuses what it must.
// Meant to be built with sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cassnat_asr_public_amd/csrc tools/ast_ngram_check.cpp -o ast_ngram_check
// Exit status 0 when every check held.
#include "ngram_check_model.h"

#include "ast_ngram_search.h"

namespace {

constexpr int EOS_TOK = 2;

// (a_word, a_eos) by a serial walk over the core alone
void ref_adds(const cn_ngram_desc& d, const std::vector<int>& row, int eos, float* out) {
    std::vector<int32_t> words = {d.bos};
    NgPiece carry = ng_piece(d, 0, false);
    for (int t : row) {
        if (t == eos || t < 0 || t >= d.vocab) continue;
        const NgPiece pc = ng_piece(d, t, true);
        if (pc.starts && carry.pw != 1) words.push_back(ng_word_id(d, carry.h));
        carry = ng_combine(carry, pc);
    }
    auto score = [&](int32_t w) {  // after `words`
        int32_t h[NG_HIST];
        const int have = (int)words.size();
        for (int i = 0; i < NG_HIST; ++i) h[NG_HIST - 1 - i] = i < have ? words[have - 1 - i] : d.bos;
        const int c = have < d.order - 1 ? have : d.order - 1;
        return ng_word_score(d, h + NG_HIST, c, w);
    };
    if (carry.pw != 1) {
        const int32_t w = ng_word_id(d, carry.h);
        const float close32 = score(w);
        words.push_back(w);
        out[0] = close32, out[1] = close32 + score(d.eos);
    } else {
        out[0] = 0.f, out[1] = score(d.eos);
    }
}

void adds_of(const cn_ngram_desc& d, const std::vector<int>& row, int eos, float* out) {
    std::unique_ptr<int32_t[]> tok(new int32_t[row.size() ? row.size() : 1]);  // exactly the row: a read behind it is a heap overflow
    for (size_t i = 0; i < row.size(); ++i) tok[i] = row[i];
    an_adds_row_host(d, tok.get(), (int)row.size(), eos, out);
}

std::vector<int> random_row(const Model& m, std::mt19937& rng, int len, bool clean) {
    std::vector<int> row;
    for (int i = 0; i < len; ++i) {
        const unsigned u = rng() % 100;
        if (!clean && u < 4) row.push_back(EOS_TOK);
        else if (!clean && u < 8) row.push_back((int)(rng() % 3 == 0 ? -1 - (int)(rng() % 9) : m.d.vocab + (int)(rng() % 9)));
        else row.push_back((int)(rng() % m.d.vocab) == EOS_TOK ? 0 : (int)(rng() % m.d.vocab));
    }
    for (int& t : row)
        if (clean && t == EOS_TOK) t = 0;
    return row;
}

void check_rows(const Model& m, std::mt19937& rng, const std::vector<uint8_t>& starts) {
    const cn_ngram_desc& d = m.d;
    const int V = d.vocab, sep = V - 1, w0 = 4;  // pieces: 4 specials, the words (each begins one), continuations, a bare separator
    std::vector<std::vector<int>> rows = {{}, {w0}, {w0 + 1, V - 2}, {V - 3, V - 2}, {w0, sep}, {sep}, {sep, sep, w0}, {EOS_TOK}, {w0, EOS_TOK, V - 2, EOS_TOK, w0 + 2},
                                          {w0, -3, V - 2, V, 1000, w0 + 1}, {-1}, {0, 1, 3, w0, 1}};
    std::vector<int> many;
    for (int i = 0; i < 11; ++i) many.push_back(w0 + i % 12);
    rows.push_back(many);
    many.push_back(sep);
    rows.push_back(many);
    for (int it = 0; it < 400; ++it) rows.push_back(random_row(m, rng, (int)(rng() % 90), false));
    for (const auto& row : rows) {
        float got[2], want[2];
        adds_of(d, row, EOS_TOK, got);
        ref_adds(d, row, EOS_TOK, want);
        CHECK(memcmp(got, want, 8) == 0, "order %d, row of %d: adds (%a, %a), core (%a, %a)", d.order, (int)row.size(), got[0], got[1], want[0], want[1]);
        // what contributes no piece changes nothing
        std::vector<int> kept;
        for (int t : row)
            if (t != EOS_TOK && t >= 0 && t < V) kept.push_back(t);
        float again[2];
        adds_of(d, kept, EOS_TOK, again);
        CHECK(memcmp(got, again, 8) == 0, "order %d: dropped ids changed the adds", d.order);
    }
    // the terms along a hypothesis sum to the ranker's score of its words and </s>
    for (int it = 0; it < 200; ++it) {
        const std::vector<int> seq = random_row(m, rng, (int)(rng() % 30), true);
        float total = 0.f, a[2];
        for (size_t i = 0; i <= seq.size(); ++i) {
            adds_of(d, std::vector<int>(seq.begin(), seq.begin() + i), EOS_TOK, a);
            total += an_term(starts.data(), a, EOS_TOK, i < seq.size() ? seq[i] : EOS_TOK, V);
        }
        // the same words scored one after the other
        std::vector<int32_t> ids(NG_HIST, d.bos);
        int before = 0;
        float want = 0.f;
        auto word = [&](int32_t w) {
            const int c = before + 1 < d.order - 1 ? before + 1 : d.order - 1;
            want += ng_word_score(d, ids.data() + ids.size(), c, w);
            ids.push_back(w);
            ++before;
        };
        NgPiece carry = ng_piece(d, 0, false);
        for (int t : seq) {
            const NgPiece pc = ng_piece(d, t, true);
            if (pc.starts && carry.pw != 1) word(ng_word_id(d, carry.h));
            carry = ng_combine(carry, pc);
        }
        if (carry.pw != 1) word(ng_word_id(d, carry.h));
        word(d.eos);
        CHECK(total == want, "order %d, %d tokens: terms sum to %a, the words to %a", d.order, (int)seq.size(), total, want);
    }
}

void check_refusals(const Model& m) {
    CHECK(ng_check_desc(m.d).empty(), "%s", ng_check_desc(m.d).c_str());
    cn_ngram_desc d = m.d;
    d.order = 0;
    CHECK(!ng_check_desc(d).empty(), "order 0 accepted");
    d.order = NG_MAX_ORDER + 1;
    CHECK(!ng_check_desc(d).empty(), "order 9 accepted");
    d = m.d, d.gram_slots = 48;
    CHECK(!ng_check_desc(d).empty(), "48 slots accepted");
    d = m.d, d.word_slots = 0;
    CHECK(!ng_check_desc(d).empty(), "0 slots accepted");
    d = m.d, d.piece_pow = nullptr;
    CHECK(!ng_check_desc(d).empty(), "null table accepted");
    d = m.d, d.vocab = -1;
    CHECK(!ng_check_desc(d).empty(), "negative vocab accepted");
}

}  // namespace

int main() {
    std::mt19937 rng(4321);
    const std::vector<std::string> words = {"ab", "ba", "abc", "c", "cc", "bca", "a", "b", "cab", "bb", "abcbc", "bc"};
    for (int order : {1, 2, 3, 5, 8}) {
        std::vector<std::string> pieces;
        std::vector<uint8_t> starts;
        const auto m = make_model(order, rng, words, &pieces, &starts);
        check_rows(*m, rng, starts);
        check_refusals(*m);
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ast_ngram_check: all checks held\n");
    return 0;
}
