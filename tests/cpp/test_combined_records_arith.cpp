// test_combined_records_arith.cpp — GT, GQ and GL per VCF record from the COMBINED bins of a group of chains, the route of
// pangenie_amd/csrc/pg_combine_records.hip on the CPU: pgc_fold per key over the chains (pg_combine.h), the key walk over the
// combined bins (pgc_record_keys_of), pgx_decide_record and pgx_record_gl (pg_calls.h) — against a long double restatement of
// what the host does: std::map sums over the chains in group order, normalise, fold onto the record's alleles,
// an empty map as L(0/0) = 1, the genotypes over undefined alleles dropped and the rest renormalised, likeliest genotype with
// >= and the 1e-10 tie rule, quality from log10l, and the digits of log10l as "%.3Le" prints them.
// GT, GQ and flag wherever the route does not defer; every GL value that is not deferred.
// Stand-alone: g++ -std=c++17 -I pangenie_amd/csrc, no device.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pg_combine.h"

static_assert(LDBL_MANT_DIG == 64, "this test needs the x87 80-bit long double");

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                      \
    } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<uint64_t> g_tm(PG_GQ_STEPS);
static std::vector<int32_t> g_te(PG_GQ_STEPS);

struct Chain {
    bool kept = true;
    std::vector<uint8_t> pres;    // [A]
    std::vector<double> m;        // [A (A + 1) / 2] bins, slot pairs a <= b in row order
    std::vector<int32_t> e;
};
struct Bubble {
    std::vector<uint16_t> id;     // [A] allele id of every slot, ascending
    std::vector<Chain> chains;    // in group order
};
struct Record {
    std::vector<uint16_t> own;    // by bubble allele ID: the record allele it carries
    std::vector<uint16_t> vcf;    // [n_alleles] index among the defined alleles, 0xFFFF: undefined
    bool has_undefined() const { for (uint16_t x : vcf) if (x == 0xFFFF) return true; return false; }
    unsigned n_defined() const { unsigned n = 0; for (uint16_t x : vcf) n += x != 0xFFFF; return n; }
};
struct Call { uint32_t flags, a1, a2, gq; };
typedef std::pair<unsigned, unsigned> G;

// ---- the host route in long double ----
struct Host {
    Call call;
    std::vector<long double> L;   // per VCF genotype (a <= b over the defined alleles) at b (b + 1) / 2 + a
    bool rule_defers;             // a key whose largest nonzero summand lies below 2^-16300
    bool has_12 = false;
};

static Host host(const Bubble& b, const Record& r) {
    const size_t A = b.id.size();
    std::map<G, long double> M, largest;       // GenotypingResult::combine over the chains, in their order
    for (const Chain& c : b.chains) {
        size_t bin = 0;
        for (size_t x = 0; x < A; ++x)
            for (size_t y = x; y < A; ++y, ++bin)
                if (c.kept && c.pres[x] && c.pres[y]) {
                    const long double v = ldexpl((long double)c.m[bin], c.e[bin]);
                    M[G(b.id[x], b.id[y])] += v;
                    long double& l = largest[G(b.id[x], b.id[y])];
                    if (v > l) l = v;
                }
    }
    Host h;
    h.rule_defers = false;
    for (auto& kv : largest) if (kv.second > 0.0L && kv.second < ldexpl(1.0L, PG_CALLS_DEFER_EXP)) h.rule_defers = true;
    long double sum = 0.0L;                     // normalize
    for (auto& kv : M) sum += kv.second;
    if (sum > 0) for (auto& kv : M) kv.second = kv.second / sum;
    std::map<G, long double> F;                 // Variant::separate_variants
    for (auto& kv : M) {
        unsigned ra = r.own[kv.first.first], rb = r.own[kv.first.second];
        if (ra > rb) std::swap(ra, rb);
        F[G(ra, rb)] += kv.second;
    }
    if (F.empty()) F[G(0, 0)] = 1.0L;
    std::map<G, long double> S;                 // get_specific_likelihoods over the defined alleles (keys: GT numbers)
    long double sum2 = 0.0L;
    for (auto& kv : F) {
        if (r.vcf[kv.first.first] == 0xFFFF || r.vcf[kv.first.second] == 0xFFFF) continue;
        S[G(r.vcf[kv.first.first], r.vcf[kv.first.second])] += kv.second;
        sum2 += kv.second;
    }
    if (r.has_undefined() && sum2 > 0) for (auto& kv : S) kv.second = kv.second / sum2;
    const unsigned nd = r.n_defined();
    h.L.assign((size_t)nd * (nd + 1) / 2, 0.0L);
    for (auto& kv : S) h.L[(size_t)kv.first.second * (kv.first.second + 1) / 2 + kv.first.first] = kv.second;
    h.has_12 = M.count(G(1, 2)) != 0;
    Call c = {PGX_CALL_NONE, 0xFFFF, 0xFFFF, 0};
    h.call = c;
    if (S.empty()) return h;
    long double best = 0.0L;                    // get_likeliest_genotype
    G bg(0, 0);
    for (auto& kv : S) if (kv.second >= best) { best = kv.second; bg = kv.first; }
    bool unique = true;
    for (auto& kv : S) if (kv.first != bg && fabsl(kv.second - best) < 0.0000000001) unique = false;
    if (!(best > 0.0L)) return h;
    if (!unique) { h.call.flags = PGX_CALL_NOT_UNIQUE; return h; }
    h.call.flags = PGX_CALL_OK;
    h.call.a1 = bg.first; h.call.a2 = bg.second;
    const long double pw = 1.0L - best;         // get_genotype_quality
    h.call.gq = pw > 0.0 ? (uint32_t)(size_t)(-10 * log10l(pw)) : 10000u;
    return h;
}

// the digits of log10l(L) as "%.3Le" prints them
static pg_gl digits_of(long double L) {
    if (!(L > 0.0L)) return pgx_gl_neg_inf();
    const long double y = log10l(L);
    if (y == 0.0L) return pgx_gl_of(0, 0);
    char buf[64];
    snprintf(buf, sizeof buf, "%.3Le", fabsl(y));   // d.ddde[+-]XX
    const int mant = (buf[0] - '0') * 1000 + (buf[2] - '0') * 100 + (buf[3] - '0') * 10 + (buf[4] - '0');
    const int ex = atoi(buf + 6);
    return pgx_gl_of(y < 0 ? -mant : mant, ex);
}

// ---- the device's route ----
static std::vector<pg_combined_bin> combine(const Bubble& b) {
    const size_t A = b.id.size();
    std::vector<pg_combined_bin> out;
    size_t bin = 0;
    for (size_t x = 0; x < A; ++x)
        for (size_t y = x; y < A; ++y, ++bin) {
            pgc_fold f;
            pgc_fold_init(&f);
            for (const Chain& c : b.chains)
                if (c.kept && c.pres[x] && c.pres[y]) pgc_fold_take(&f, pgc_summand(c.m[bin], c.e[bin]));
            out.push_back(pgc_fold_bin(&f));
        }
    return out;
}

struct DefinedOf {
    const Record* r;
    bool operator()(uint32_t a) const { return r->vcf[a] != 0xFFFF; }
};
struct VcfOf {
    const Record* r;
    uint32_t operator()(uint32_t a) const { return r->vcf[a]; }
};
struct Store {
    std::vector<pg_gl>* out;
    void operator()(uint32_t i, pg_gl g) const { (*out)[i] = g; }
};

struct Route {
    Call call;
    std::vector<pg_gl> gl;
    bool deferred;   // a PG_COMBINED_DEFERRED bin: the whole variant
};

template <class Keys>
static Route decide(Keys& keys, const Record& r, bool deferred) {
    Route o;
    o.deferred = deferred;
    const unsigned nd = r.n_defined();
    o.gl.assign((size_t)nd * (nd + 1) / 2, pgx_gl_deferred());
    Call c = {PGX_CALL_DEFERRED, 0xFFFF, 0xFFFF, 0};
    o.call = c;
    if (deferred) return o;
    DefinedOf def = {&r};
    const pgx_record_decision d = pgx_decide_record(keys, r.has_undefined(), def, g_tm.data(), g_te.data());
    o.call.flags = d.flags;
    if ((d.flags & 0xFFu) == PGX_CALL_OK) { o.call.a1 = r.vcf[d.key >> 16]; o.call.a2 = r.vcf[d.key & 0xFFFFu]; o.call.gq = d.gq; }
    VcfOf vcf = {&r};
    Store st = {&o.gl};
    pgx_record_gl(keys, (uint32_t)r.vcf.size(), r.has_undefined(), vcf, st);
    return o;
}

static Route route(const Bubble& b, const Record& r, const std::vector<pg_combined_bin>& bins) {
    const uint32_t A = (uint32_t)b.id.size();
    std::vector<uint16_t> own(A);
    for (uint32_t s = 0; s < A; ++s) own[s] = r.own[b.id[s]];
    if (A <= 8) {   // the lane-per-record kernels' walk: a byte per slot
        pgc_record_keys keys;
        keys.bins = bins.data(); keys.A = A; keys.own.w = 0;
        for (uint32_t s = 0; s < A; ++s) keys.own.w |= (unsigned long long)(own[s] & 0xFFu) << (8u * s);
        return decide(keys, r, keys.any_deferred());
    }
    pgc_record_keys_of<pgc_own_array> keys;
    keys.bins = bins.data(); keys.A = A; keys.own.of_slot = own.data();
    return decide(keys, r, keys.any_deferred());
}

// the walk of ONE chain's bins as the record calls of single chains do it: presence from the allele mask, pgx_from_bin
struct ChainKeys {
    const Bubble* b;
    const Chain* c;
    const Record* r;
    size_t x, y, bin;
    void start() { x = 0; y = 0; bin = 0; }
    bool next(pgx* v, uint32_t* key) {
        const size_t A = b->id.size();
        while (x < A) {
            const size_t cx = x, cy = y, cbin = bin;
            ++bin;
            if (++y == A) { ++x; y = x; }
            if (c->kept && c->pres[cx] && c->pres[cy]) {
                uint32_t ra = r->own[b->id[cx]], rb = r->own[b->id[cy]];
                if (ra > rb) std::swap(ra, rb);
                *v = pgx_from_bin(c->m[cbin], c->e[cbin]);
                *key = (ra << 16) | rb;
                return true;
            }
        }
        return false;
    }
};

static std::string text_of(pg_gl g) {
    char buf[32];
    return pgx_gl_text(g, buf, sizeof buf) >= 0 ? buf : "?";
}

static long g_records = 0, g_deferred_records = 0, g_values = 0, g_deferred_values = 0;

// compares one record; answers the route's result
static Route check(const Bubble& b, const Record& r, const char* what) {
    const std::vector<pg_combined_bin> bins = combine(b);
    const Host want = host(b, r);
    const Route got = route(b, r, bins);
    ++g_records;
    if (want.rule_defers) CHECK(got.deferred && got.call.flags == PGX_CALL_DEFERRED, "%s: a key below the cut does not defer the variant", what);
    CHECK(got.gl.size() == want.L.size(), "%s: %zu values, %zu expected", what, got.gl.size(), want.L.size());
    if ((got.call.flags & 0xFFu) == PGX_CALL_DEFERRED) ++g_deferred_records;
    else
        CHECK((got.call.flags & 0xFFu) == want.call.flags && got.call.a1 == want.call.a1 && got.call.a2 == want.call.a2 && got.call.gq == want.call.gq,
              "%s: A %zu, %zu chains: flags %#x GT %u/%u GQ %u, long double: flags %u GT %u/%u GQ %u", what, b.id.size(), b.chains.size(), got.call.flags,
              got.call.a1, got.call.a2, got.call.gq, want.call.flags, want.call.a1, want.call.a2, want.call.gq);
    for (size_t i = 0; i < got.gl.size() && i < want.L.size(); ++i) {
        ++g_values;
        if (pgx_gl_is_deferred(got.gl[i])) { ++g_deferred_values; continue; }
        const pg_gl w = digits_of(want.L[i]);
        char txt[64];
        snprintf(txt, sizeof txt, "%.4Lg", want.L[i] > 0.0L ? log10l(want.L[i]) : -INFINITY);
        CHECK(got.gl[i].mant == w.mant && got.gl[i].exp10 == w.exp10 && text_of(got.gl[i]) == txt,
              "%s: value %zu is %d e%d \"%s\", long double: %d e%d \"%s\"", what, i, got.gl[i].mant, got.gl[i].exp10, text_of(got.gl[i]).c_str(), w.mant,
              w.exp10, txt);
    }
    return got;
}

static double rnd_mant() { return ldexp((double)((rnd() >> 11) | (1ull << 52)), -53); }

static Record rnd_record(unsigned n_ids) {
    Record r;
    const unsigned nA = 1 + rnd() % (n_ids < 6 ? n_ids : 6);
    r.own.resize(n_ids);
    for (unsigned i = 0; i < n_ids; ++i) r.own[i] = (uint16_t)(i == 0 ? 0 : rnd() % nA);
    r.vcf.resize(nA);
    uint16_t d = 0;
    for (unsigned a = 0; a < nA; ++a) r.vcf[a] = (a == 0 || rnd() % 10 != 0) ? d++ : (uint16_t)0xFFFF;   // a tenth undefined
    return r;
}

static void test_random(int n) {
    long one_chain = 0;
    for (int it = 0; it < n; ++it) {
        Bubble b;
        const unsigned pick = rnd() % 100;
        const unsigned A = pick < 80 ? 1 + rnd() % 5 : (pick < 98 ? 6 + rnd() % 7 : 40), S = 1 + rnd() % 4;
        const unsigned spread = (rnd() % 4 == 0) ? 401 : (rnd() % 2 ? 8 : 70);
        uint16_t id = 0;
        for (unsigned a = 0; a < A; ++a) { b.id.push_back(id); id += 1 + (rnd() % 5 == 0); }
        const bool near_cut = rnd() % 50 == 0;
        const int32_t base = near_cut ? -16200 - (int32_t)(rnd() % 200) : -(int32_t)(rnd() % 9000);
        for (unsigned s = 0; s < S; ++s) {
            Chain c;
            c.kept = rnd() % 20 != 0;
            for (unsigned a = 0; a < A; ++a) c.pres.push_back(rnd() % 4 != 0);
            const int32_t shift = (int32_t)(rnd() % 3 == 0 ? rnd() % 60 : 0);
            for (unsigned k = 0; k < A * (A + 1) / 2; ++k) {
                c.m.push_back(rnd() % 13 == 0 ? 0.0 : rnd_mant());
                c.e.push_back(base - shift - (int32_t)(rnd() % spread));
            }
            b.chains.push_back(c);
        }
        const unsigned n_rec = 1 + rnd() % 3;
        for (unsigned q = 0; q < n_rec; ++q) {
            const Record r = rnd_record(id);
            const Route got = check(b, r, "random");
            if (S == 1 && !near_cut) {   // a group of ONE chain: the walk over the combined bins IS the walk over the chain's
                ChainKeys keys = {&b, &b.chains[0], &r, 0, 0, 0};
                const Route one = decide(keys, r, false);
                ++one_chain;
                bool same = one.call.flags == got.call.flags && one.call.a1 == got.call.a1 && one.call.a2 == got.call.a2 && one.call.gq == got.call.gq &&
                            one.gl.size() == got.gl.size();
                for (size_t i = 0; same && i < one.gl.size(); ++i) same = one.gl[i].mant == got.gl[i].mant && one.gl[i].exp10 == got.gl[i].exp10;
                CHECK(same, "one chain, A %u: the combined route differs from the chain's own (flags %#x / %#x)", A, got.call.flags, one.call.flags);
            }
        }
    }
    CHECK(one_chain > n / 8, "only %ld records of one-chain groups", one_chain);
}

// ---- constructed cases ----
static Chain chain(std::vector<uint8_t> pres, std::vector<double> m, std::vector<int32_t> e, bool kept = true) {
    Chain c;
    c.kept = kept; c.pres = pres; c.m = m; c.e = e;
    return c;
}
static Record record(std::vector<uint16_t> own, std::vector<uint16_t> vcf) {
    Record r;
    r.own = own; r.vcf = vcf;
    return r;
}
static bool is_neg_inf(pg_gl g) { return g.mant == 0 && g.exp10 == PG_GL_NEG_INF; }

static void test_constructed() {
    const std::vector<int32_t> z6(6, 0);
    const std::vector<uint16_t> ids3 = {0, 1, 2};
    // the union rule: subsets that carry {0,1} and {0,2} give no key (1,2)
    {
        Bubble b;
        b.id = ids3;
        b.chains.push_back(chain({1, 1, 0}, {0.25, 0.125, 9, 0.0625, 9, 9}, z6));
        b.chains.push_back(chain({1, 0, 1}, {0.125, 9, 0.25, 9, 9, 0.03125}, z6));
        const std::vector<pg_combined_bin> bins = combine(b);
        CHECK(bins[4].flags == 0 && bins[4].m == 0, "the union of {0,1} and {0,2} holds a key (1,2)");
        CHECK(bins[0].flags == PG_COMBINED_PRESENT && pgx_to_ld(pgx{bins[0].m, bins[0].e}) == 0.375L, "key (0,0) is not the sum of both subsets");
        const Record r = record({0, 1, 2}, {0, 1, 2});
        CHECK(!host(b, r).has_12, "the yardstick holds a key (1,2)");
        const Route got = check(b, r, "union rule");
        CHECK(got.gl.size() == 6 && is_neg_inf(got.gl[4]) && !is_neg_inf(got.gl[3]) && !is_neg_inf(got.gl[5]), "the pair 1/2 has a likelihood");
        check(b, record({0, 1, 1}, {0, 1}), "union rule, 1 and 2 onto one allele");
        check(b, record({0, 1, 2}, {0, 0xFFFF, 1}), "union rule, allele 1 undefined");
    }
    // no chain holds any key
    {
        Bubble b;
        b.id = ids3;
        b.chains.push_back(chain({1, 1, 1}, {0.25, 0.375, 0.1875, 0, 0.125, 0.0625}, z6, false));
        b.chains.push_back(chain({0, 0, 0}, {0.25, 0.375, 0.1875, 0, 0.125, 0.0625}, z6));
        const Route got = check(b, record({0, 1, 0}, {0, 1}), "no key");
        CHECK(got.call.flags == (PGX_CALL_OK | PGX_CALL_EMPTY) && got.call.a1 == 0 && got.call.a2 == 0 && got.call.gq == 10000, "no key: flags %#x", got.call.flags);
        CHECK(got.gl.size() == 3 && got.gl[0].mant == 0 && got.gl[0].exp10 == 0 && is_neg_inf(got.gl[1]) && is_neg_inf(got.gl[2]), "no key: GL is not 0, -inf, -inf");
    }
    // every held value 0
    {
        Bubble b;
        b.id = ids3;
        b.chains.push_back(chain({1, 1, 1}, {0, 0, 0, 0, 0, 0}, z6));
        b.chains.push_back(chain({1, 1, 0}, {0, 0, 0, 0, 0, 0}, z6));
        const Route got = check(b, record({0, 1, 0}, {0, 1}), "all zero");
        bool all_inf = true;
        for (pg_gl g : got.gl) all_inf = all_inf && is_neg_inf(g);
        CHECK(got.call.flags == PGX_CALL_NONE && all_inf && got.gl.size() == 3, "all zero: flags %#x", got.call.flags);
    }
    // one deferred key among large ones: the whole variant, not its neighbour
    {
        Bubble b;
        b.id = ids3;
        b.chains.push_back(chain({1, 1, 1}, {0.5, 0.75, 0.5, 0.5, 0.5, 0.5}, {-10, -12, -11, -16320, -13, -12}));
        b.chains.push_back(chain({1, 1, 1}, {0.5, 0.75, 0.5, 0.5, 0.5, 0.5}, {-11, -12, -14, -16400, -13, -12}));
        const std::vector<pg_combined_bin> bins = combine(b);
        CHECK(bins[3].flags == (PG_COMBINED_PRESENT | PG_COMBINED_DEFERRED) && bins[2].flags == PG_COMBINED_PRESENT, "the key below the cut is not flagged");
        for (const Record& r : {record({0, 1, 0}, {0, 1}), record({0, 1, 2}, {0, 0xFFFF, 1}), record({0, 0, 0}, {0})}) {
            const Route got = check(b, r, "a deferred key");
            bool all = got.call.flags == PGX_CALL_DEFERRED;
            for (pg_gl g : got.gl) all = all && pgx_gl_is_deferred(g);
            CHECK(all && got.deferred, "a deferred key: a record or a value of the variant is decided");
        }
        Bubble nb = b;
        nb.chains[0].e[3] = -14;   // the neighbour: the same bubble with that key large in one chain (0 + large: the small summand is not the largest)
        const Route got = check(nb, record({0, 1, 0}, {0, 1}), "the neighbour of a deferred variant");
        bool any = false;
        for (pg_gl g : got.gl) any = any || pgx_gl_is_deferred(g);
        CHECK(!got.deferred && got.call.flags != PGX_CALL_DEFERRED && !any, "the neighbour is deferred");
    }
    // the order example of pg_combine.h, (mid + tiny) + large, carried through to a record
    {
        Bubble b;
        b.id = {0, 1};
        const double tiny = 1.0 + 0x1p-20;
        b.chains.push_back(chain({1, 1}, {1.0, 1.0, 1.0}, {-16364, -16298, -16299}));
        b.chains.push_back(chain({1, 1}, {tiny, 1.0, 1.0}, {-16428, -16290, -16297}));
        b.chains.push_back(chain({1, 1}, {1.0, 1.0, 1.0}, {-16300, -16299, -16296}));
        const std::vector<pg_combined_bin> bins = combine(b);
        CHECK(bins[0].flags == PG_COMBINED_PRESENT && bins[0].m == PGX_TOP && bins[0].e == -16300 - 63, "(mid + tiny) + large is not large: m %llx e %d",
              (unsigned long long)bins[0].m, bins[0].e);
        const Route got = check(b, record({0, 1}, {0, 1}), "(mid + tiny) + large");
        CHECK(!got.deferred && (got.call.flags & 0xFFu) != PGX_CALL_DEFERRED, "(mid + tiny) + large is deferred");
        check(b, record({0, 0}, {0}), "(mid + tiny) + large, one allele");
    }
    // a group of ONE chain equals that chain's own walk, bit for bit (ids that are not slots, an absent allele in the middle)
    {
        Bubble b;
        b.id = {0, 2, 5, 7};
        b.chains.push_back(chain({1, 0, 1, 1}, {0.125, 9, 0.125, 0, 9, 9, 9, 0.25, 0.5, 0}, std::vector<int32_t>(10, 0)));
        const Record r = record({0, 9, 1, 9, 9, 1, 9, 2}, {0, 1, 0xFFFF});
        const Route got = check(b, r, "one chain");
        ChainKeys keys = {&b, &b.chains[0], &r, 0, 0, 0};
        const Route one = decide(keys, r, false);
        bool same = one.call.flags == got.call.flags && one.call.a1 == got.call.a1 && one.call.a2 == got.call.a2 && one.call.gq == got.call.gq && one.gl.size() == got.gl.size();
        for (size_t i = 0; same && i < one.gl.size(); ++i) same = one.gl[i].mant == got.gl[i].mant && one.gl[i].exp10 == got.gl[i].exp10;
        CHECK(same && got.call.flags == PGX_CALL_OK && got.call.a1 == 1 && got.call.a2 == 1 && got.call.gq == 3, "one chain: flags %#x GT %u/%u GQ %u", got.call.flags,
              got.call.a1, got.call.a2, got.call.gq);
    }
}

int main(int argc, char** argv) {
    if (pgx_build_gq_table(g_tm.data(), g_te.data()) != 0) { printf("the GQ table could not be built\n"); return 2; }
    const int n = argc > 1 ? atoi(argv[1]) : 200000;
    test_random(n);
    test_constructed();
    // away from the cut the route defers next to nothing: GL values alone, by the window rule (about 2e-9 of them)
    printf("%ld records (%ld deferred), %ld GL values (%ld deferred)\n", g_records, g_deferred_records, g_values, g_deferred_values);
    CHECK(g_deferred_records * 20 < g_records && g_deferred_values * 20 < g_values, "the route defers more than a twentieth");
    printf("%ld checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
