// parakeet.cpp_amd/csrc/ngram_lm.cpp -- ARPA parser and back-off automaton of the n-gram language model (ngram_lm.hpp).
#include "ngram_lm.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

#include "common.hpp"

namespace pk {

namespace {

struct Key {
    int32_t w[kLmMaxOrder];                             // unused places: -1 (so the order is part of the key)
    bool operator==(const Key &o) const { return std::memcmp(w, o.w, sizeof w) == 0; }
};
struct KeyHash {
    size_t operator()(const Key &k) const {
        uint64_t h = 0x243F6A8885A308D3ull;
        for (int i = 0; i < kLmMaxOrder; ++i) {
            h += 0x9E3779B97F4A7C15ull * (uint64_t)(uint32_t)(k.w[i] + 2);
            h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
            h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
            h ^= h >> 31;
        }
        return (size_t)h;
    }
};
struct Entry {
    Key k;
    float lp, bo;
    int32_t order, prefix;                              // prefix: entry index of the first order - 1 words (-1 for a unigram)
};

Key suffix_key(const Key &k, int order, int len) {      // the last len words of an n-gram of `order` words
    Key s;
    for (int i = 0; i < kLmMaxOrder; ++i) s.w[i] = i < len ? k.w[order - len + i] : -1;
    return s;
}

struct Tok { const char *p; int n; };

bool tok_is(const Tok &t, const char *s) { return (int)std::strlen(s) == t.n && std::memcmp(t.p, s, t.n) == 0; }

float parse_value(const Tok &t, int line, const char *what) {
    char buf[64];
    if (t.n <= 0 || t.n >= (int)sizeof buf) fail(PK_ERR_INVALID, "ARPA line %d: %s is not a number", line, what);
    std::memcpy(buf, t.p, t.n);
    buf[t.n] = 0;
    char *end = nullptr;
    const double d = std::strtod(buf, &end);
    if (end != buf + t.n) fail(PK_ERR_INVALID, "ARPA line %d: %s '%s' is not a number", line, what, buf);
    const double nat = d * 2.302585092994046;           // log10 -> natural log, in double; rounded once below
    const float f = (float)nat;
    if (!std::isfinite(d) || !std::isfinite(f)) fail(PK_ERR_INVALID, "ARPA line %d: %s '%s' is not finite in fp32", line, what, buf);
    return f;
}

int parse_word(const Tok &t, int line) {
    if (tok_is(t, "<s>")) return kLmBos;
    if (tok_is(t, "</s>")) return kLmEos;
    if (tok_is(t, "<unk>")) return kLmUnk;
    int64_t v = 0;
    bool ok = t.n > 0;
    for (int i = 0; i < t.n && ok; ++i) {
        ok = t.p[i] >= '0' && t.p[i] <= '9';
        if (ok && v < ((int64_t)1 << 40)) v = v * 10 + (t.p[i] - '0');
    }
    if (!ok) fail(PK_ERR_INVALID, "ARPA line %d: word '%.*s' is neither a decimal token id nor <s>, </s>, <unk>", line, std::min(t.n, 40), t.p);
    if (v >= kLmMaxId) fail(PK_ERR_INVALID, "ARPA line %d: token id %.*s is not below 2^24", line, std::min(t.n, 40), t.p);
    return (int)v;
}

// "ngram k=c" -> true (k, c filled)
bool parse_count(const char *p, const char *e, int &k, int64_t &c) {
    if (e - p < 9 || std::memcmp(p, "ngram", 5) != 0 || (p[5] != ' ' && p[5] != '\t')) return false;
    p += 5;
    while (p < e && (*p == ' ' || *p == '\t')) ++p;
    int64_t a = 0, b = 0;
    int na = 0, nb = 0;
    for (; p < e && *p >= '0' && *p <= '9' && na < 4; ++p, ++na) a = a * 10 + (*p - '0');
    if (!na || p >= e || *p != '=') return false;
    ++p;
    for (; p < e && *p >= '0' && *p <= '9' && nb < 15; ++p, ++nb) b = b * 10 + (*p - '0');
    if (!nb || p != e) return false;
    k = (int)a; c = b;
    return true;
}

}  // namespace

void lm_parse_arpa(const char *text, size_t n_bytes, NgramLm &out) {
    if (!text) fail(PK_ERR_INVALID, "ARPA text is null");
    out = NgramLm();
    std::vector<Entry> ent;
    std::unordered_map<Key, int32_t, KeyHash> index;
    std::vector<int64_t> declared, seen;
    std::vector<uint8_t> has_uni, named;                // grown with the ids met
    enum { M_HEAD, M_COUNTS, M_SECTION, M_DONE } mode = M_HEAD;
    int section = 0, line = 0;
    const char *p = text, *const end = text + n_bytes;
    auto close_section = [&]() {                        // the section that just ended holds what \data\ declared
        if (section > 0 && seen[section - 1] != declared[section - 1])
            fail(PK_ERR_INVALID, "ARPA line %d: the %d-grams section holds %lld entries, \\data\\ declares ngram %d=%lld", line, section,
                 (long long)seen[section - 1], section, (long long)declared[section - 1]);
    };
    while (p < end && mode != M_DONE) {
        const char *nl = (const char *)std::memchr(p, '\n', (size_t)(end - p));
        const char *b = p, *e = nl ? nl : end;
        p = nl ? nl + 1 : end;
        ++line;
        while (b < e && (*b == ' ' || *b == '\t' || *b == '\r')) ++b;
        while (e > b && (e[-1] == ' ' || e[-1] == '\t' || e[-1] == '\r')) --e;
        if (b == e) continue;
        const Tok whole{b, (int)std::min<ptrdiff_t>(e - b, 1 << 20)};
        if (mode == M_HEAD) {                        // (ARPA files may carry a free-text header in front of \data\)
            if (tok_is(whole, "\\data\\")) mode = M_COUNTS;
            continue;
        }
        if (*b == '\\') {
            if (mode == M_SECTION) close_section();
            if (tok_is(whole, "\\end\\")) {
                if (section != (int)declared.size() || declared.empty())
                    fail(PK_ERR_INVALID, "ARPA line %d: \\end\\ after %d of the %d declared sections", line, section, (int)declared.size());
                mode = M_DONE;
                continue;
            }
            int k = 0;
            bool ok = e - b >= 9 && e - b <= 10 && std::memcmp(e - 7, "-grams:", 7) == 0;
            for (const char *q = b + 1; ok && q < e - 7; ++q) { ok = *q >= '0' && *q <= '9'; k = k * 10 + (*q - '0'); }
            if (!ok) fail(PK_ERR_INVALID, "ARPA line %d: unknown section '%.*s'", line, std::min(whole.n, 40), b);
            if (k != section + 1 || k > (int)declared.size())
                fail(PK_ERR_INVALID, "ARPA line %d: section \\%d-grams: where \\%d-grams: of %d declared orders belongs", line, k, section + 1, (int)declared.size());
            section = k;
            mode = M_SECTION;
            continue;
        }
        if (mode == M_COUNTS) {
            int k = 0;
            int64_t c = 0;
            if (!parse_count(b, e, k, c)) fail(PK_ERR_INVALID, "ARPA line %d: expected 'ngram k=count'", line);
            if (k != (int)declared.size() + 1 || k > kLmMaxOrder)
                fail(PK_ERR_INVALID, "ARPA line %d: 'ngram %d=' where order %d belongs (orders 1..%d are supported)", line, k, (int)declared.size() + 1, kLmMaxOrder);
            declared.push_back(c);
            seen.push_back(0);
            continue;
        }
        // an n-gram of the current section: value, `section` words, an optional back-off
        Tok t[kLmMaxOrder + 3];
        int nt = 0;
        for (const char *q = b; q < e;) {
            while (q < e && (*q == ' ' || *q == '\t')) ++q;
            const char *w = q;
            while (q < e && *q != ' ' && *q != '\t') ++q;
            if (q > w) {
                if (nt == kLmMaxOrder + 2) { nt = kLmMaxOrder + 3; break; }
                t[nt++] = Tok{w, (int)std::min<ptrdiff_t>(q - w, 1 << 20)};
            }
        }
        if (nt != section + 1 && nt != section + 2) fail(PK_ERR_INVALID, "ARPA line %d: a %d-gram needs a value, %d words and at most one back-off", line, section, section);
        Entry en;
        en.order = section;
        en.lp = parse_value(t[0], line, "the log-probability");
        en.bo = nt == section + 2 ? parse_value(t[section + 1], line, "the back-off weight") : 0.0f;
        for (int i = 0; i < kLmMaxOrder; ++i) en.k.w[i] = i < section ? parse_word(t[1 + i], line) : -1;
        for (int i = 0; i < section; ++i) {
            const int c = en.k.w[i];
            if (c >= kLmMaxId) continue;
            if ((size_t)c >= named.size()) { named.resize((size_t)c + 1, 0); has_uni.resize((size_t)c + 1, 0); }
            if (section > 1 && !has_uni[c] && !out.has_unk)
                fail(PK_ERR_INVALID, "ARPA line %d: token id %d has no unigram and the model has no <unk>", line, c);
            named[c] = 1;
        }
        en.prefix = -1;
        if (section > 1) {
            Key pre = en.k;
            pre.w[section - 1] = -1;
            auto it = index.find(pre);
            if (it == index.end()) fail(PK_ERR_INVALID, "ARPA line %d: the first %d words of this %d-gram are not an entry themselves", line, section - 1, section);
            en.prefix = it->second;
        }
        if (ent.size() >= (size_t)0x7ffffff0) fail(PK_ERR_INVALID, "ARPA line %d: too many n-grams", line);
        if (!index.emplace(en.k, (int32_t)ent.size()).second) fail(PK_ERR_INVALID, "ARPA line %d: duplicate n-gram", line);
        if (section == 1) {
            const int c = en.k.w[0];
            if (c < kLmMaxId) has_uni[c] = 1;
            else if (c == kLmUnk) { out.has_unk = true; out.unk_lp = en.lp; }
            else if (c == kLmBos) out.has_bos = true;
            else { out.has_eos = true; }
        }
        ent.push_back(en);
        ++seen[section - 1];
    }
    if (mode == M_HEAD) fail(PK_ERR_INVALID, "ARPA line %d: no \\data\\ section", line);
    if (mode != M_DONE) fail(PK_ERR_INVALID, "ARPA line %d: the text ends before \\end\\", line);

    // ---- the automaton --------------------------------------------------------------------------------------------------
    const int n = (int)declared.size();
    out.order = n;
    out.counts = seen;
    size_t n_ctx = 0;                                   // entries of order < n come first (sections are in order): entry i is state 1 + i
    for (int k = 0; k + 1 < n; ++k) n_ctx += (size_t)seen[k];
    auto state_of_suffix = [&](const Key &k, int order, int from_len) -> int32_t {   // the longest suffix of <= from_len words that is a state
        for (int len = std::min(from_len, n - 1); len >= 1; --len) {
            auto it = index.find(suffix_key(k, order, len));
            if (it != index.end()) return it->second + 1;
        }
        return 0;
    };
    out.state.assign(n_ctx + 1, LmState{0, 0, 0.0f, 0});
    for (size_t i = 0; i < n_ctx; ++i) {
        out.state[i + 1].bo = ent[i].bo;
        out.state[i + 1].bo_state = state_of_suffix(ent[i].k, ent[i].order, ent[i].order - 1);
    }
    const int U = (int)named.size();
    out.named = named;
    out.has_uni = has_uni;
    out.uni.assign((size_t)U, LmArc{out.unk_lp, 0});
    std::vector<std::pair<uint64_t, int32_t>> ord;      // (prefix state << 32 | symbol, entry) of every entry of order >= 2
    ord.reserve(ent.size() - (size_t)seen[0]);
    for (size_t i = 0; i < ent.size(); ++i) {
        const Entry &en = ent[i];
        const int c = en.k.w[en.order - 1];
        if (en.order == 1) {
            const LmArc a{en.lp, state_of_suffix(en.k, 1, 1)};
            if (c < kLmMaxId) out.uni[c] = a;
            else if (c == kLmEos) out.eos_uni = a;
            else if (c == kLmBos) out.start = a.next;
            continue;
        }
        ord.emplace_back(((uint64_t)(uint32_t)(en.prefix + 1) << 32) | (uint32_t)c, (int32_t)i);
    }
    std::sort(ord.begin(), ord.end());
    out.arc_tok.resize(ord.size());
    out.arc.resize(ord.size());
    for (size_t a = 0; a < ord.size(); ++a) {
        const Entry &en = ent[ord[a].second];
        const int32_t s = (int32_t)(ord[a].first >> 32);
        if (out.state[s].arc_n++ == 0) out.state[s].arc_lo = (int32_t)a;
        out.arc_tok[a] = (int32_t)(uint32_t)ord[a].first;
        out.arc[a] = LmArc{en.lp, state_of_suffix(en.k, en.order, en.order)};
    }
}

bool NgramLm::lookup(int s, int c, float &lp, int &next) const {
    float acc = 0.0f;
    while (s != 0) {
        const LmState &st = state[s];
        const int32_t *lo = arc_tok.data() + st.arc_lo, *hi = lo + st.arc_n;
        const int32_t *it = std::lower_bound(lo, hi, (int32_t)c);
        if (it != hi && *it == c) {
            const LmArc &a = arc[it - arc_tok.data()];
            lp = acc + a.lp;
            next = a.next;
            return true;
        }
        acc = acc + st.bo;
        s = st.bo_state;
    }
    LmArc a{unk_lp, 0};
    if (c >= 0 && c < U() && (has_uni[c] || has_unk)) a = uni[c];
    else if (c == kLmEos && has_eos) a = eos_uni;
    else if (!has_unk) return false;
    lp = acc + a.lp;
    next = a.next;
    return true;
}

float lm_score_string(const NgramLm &lm, const int32_t *ids, int n, bool bos, bool eos) {
    int s = bos ? lm.start : 0;
    float sum = 0.0f;
    for (int k = 0; k < n + (eos ? 1 : 0); ++k) {
        const int c = k < n ? ids[k] : kLmEos;
        if (c < 0 || (k < n && c >= kLmMaxId)) fail(PK_ERR_INVALID, "token id %d at position %d is outside 0 .. 2^24 - 1", c, k);
        float lp = 0.0f;
        int next = 0;
        if (!lm.lookup(s, c, lp, next))
            fail(PK_ERR_INVALID, "%s at position %d has no unigram and the model has no <unk>", k < n ? "the token id" : "</s>", k);
        sum = sum + lp;
        s = next;
    }
    return sum;
}

void lm_check_vocab(const NgramLm &lm, int V, int blank) {
    if (lm.U() > V) fail(PK_ERR_INVALID, "the language model names token id %d, the vocabulary has %d entries", lm.U() - 1, V);
    if (blank >= 0 && blank < lm.U() && lm.named[blank]) fail(PK_ERR_INVALID, "the language model names the blank id %d", blank);
    if (lm.has_unk) return;
    for (int c = 0; c < V; ++c)
        if (c != blank && (c >= lm.U() || !lm.has_uni[c]))
            fail(PK_ERR_INVALID, "the language model has neither <unk> nor a unigram for token id %d of the vocabulary", c);
}

}  // namespace pk
