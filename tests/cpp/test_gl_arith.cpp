// test_gl_arith.cpp — pgx_gl and pgx_record_gl (pangenie_amd/csrc/pg_calls.h), the GL column of the VCF formed from integer
// pairs and an fp64 logarithm, against the machine's long double: every value that is not PG_GL_DEFERRED must print what
// snprintf("%.4Lg", log10l(x)) prints.  That is a condition, not a measurement.
//   test_gl_arith.bin [n_random [search]]     n_random: random pairs (default 10^7); "search": also look for a fold > 1
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

#include "pg_calls.h"

static_assert(LDBL_MANT_DIG == 64, "this test needs the x87 80-bit long double");
static_assert(sizeof(pg_gl) == 4, "a GL value is 4 bytes");

static int g_fail = 0;
static long g_checks = 0, g_deferred = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                      \
    } while (0)

static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::string text_ld(long double x) {   // what the host prints
    char buf[64];
    snprintf(buf, sizeof buf, "%.4Lg", log10l(x));
    return buf;
}
static std::string text_gl(pg_gl g) {
    char buf[32];
    return pgx_gl_text(g, buf, sizeof buf) < 0 ? "?" : buf;
}

// one value: decided and equal, or deferred; answers whether it was deferred
static bool check_value(pgx x, const char* what) {
    const pg_gl g = pgx_gl(x);
    if (pgx_gl_is_deferred(g)) { ++g_deferred; return true; }
    const std::string want = text_ld(pgx_to_ld(x)), got = text_gl(g);
    CHECK(got == want, "%s: m %#llx e %d: \"%s\", long double prints \"%s\"", what, (unsigned long long)x.m, x.e, got.c_str(), want.c_str());
    return false;
}

static pgx pair(uint64_t m, int32_t e) { pgx x; x.m = m; x.e = e; return x; }

static void test_constants() {
    const long double l2 = log10l(2.0L);
    CHECK(fabsl(((long double)PGX_LOG10_2_HI - l2) + (long double)PGX_LOG10_2_LO) < 0x1p-62L, "log10 2 = c_hi + c_lo");
    CHECK(ldexp(PGX_LOG10_2_HI, 39) == floor(ldexp(PGX_LOG10_2_HI, 39)), "c_hi has 37 bits: E c_hi is exact");
    CHECK((long double)PGX_LN_10 == (long double)(double)logl(10.0L), "ln 10");
    CHECK(16.0 * (16.0 * 0x1p-53 * 1e4) <= PG_GL_WINDOW, "the window is at least 16 times the error bound of s");
}

static void test_random(long n) {
    long deferred = 0;
    for (long i = 0; i < n; ++i) {
        const uint64_t r = rnd();
        uint64_t m = rnd() | PGX_TOP;
        switch (i & 3) {
        case 0: deferred += check_value(pair(m, -64 - (int32_t)(r % 16300)), "whole range"); break;              // E in [-16299, 0]
        case 1: deferred += check_value(pair(m, -64 - (int32_t)(r % 40)), "x in [2^-40, 1)"); break;
        case 2: {   // 1 - d 2^-64, d in [1, 2^63] of every magnitude
            uint64_t d = (rnd() >> (r % 64));
            if (d == 0) d = 1;
            if (d > PGX_TOP) d = PGX_TOP;
            deferred += check_value(pair(0ull - d, -64), "1 - d 2^-64");
            break;
        }
        default: {  // 1 + d 2^-63, d in [1, 2^63)
            uint64_t d = (rnd() >> (1 + r % 63));
            if (d == 0) d = 1;
            deferred += check_value(pair(PGX_TOP + d, -63), "1 + d 2^-63");
        }
        }
    }
    printf("random: %ld values, %ld deferred\n", n, deferred);
    CHECK((double)deferred <= 1e-6 * (double)n, "%ld of %ld random values deferred: more than 1e-6", deferred, n);
}

static void test_special() {
    CHECK(text_gl(pgx_gl(pgx_one())) == "0" && text_ld(1.0L) == "0", "x = 1");
    CHECK(text_gl(pgx_gl(pgx_zero())) == "-inf" && text_ld(0.0L) == "-inf", "x = 0");
    const pg_gl one = pgx_gl(pgx_one()), zero = pgx_gl(pgx_zero());
    CHECK(one.mant == 0 && one.exp10 == 0 && zero.mant == 0 && zero.exp10 == PG_GL_NEG_INF, "the encodings of 1 and 0");
    // both sides of 2^-16300
    const pgx at = pair(PGX_TOP, PG_CALLS_DEFER_EXP - 63), below = pair(~0ull, PG_CALLS_DEFER_EXP - 64);
    CHECK(!pgx_gl_is_deferred(pgx_gl(at)), "2^-16300 is decided");
    check_value(at, "2^-16300");
    CHECK(text_gl(pgx_gl(at)) == "-4907", "2^-16300 prints -4907, not %s", text_gl(pgx_gl(at)).c_str());
    CHECK(pgx_gl_is_deferred(pgx_gl(below)), "the largest value below 2^-16300 is deferred");
    CHECK(pgx_gl_is_deferred(pgx_gl(pair(PGX_TOP, -16400))), "a value far below 2^-16300 is deferred");
    // the largest and smallest logarithms next to 1, and the sign
    check_value(pair(~0ull, -64), "1 - 2^-64");
    check_value(pair(PGX_TOP + 1, -63), "1 + 2^-63");
    CHECK(text_gl(pgx_gl(pair(PGX_TOP + 1, -63))) == "4.709e-20", "1 + 2^-63 prints 4.709e-20, not %s", text_gl(pgx_gl(pair(PGX_TOP + 1, -63))).c_str());
    CHECK(pgx_gl(pair(~0ull, -64)).mant < 0 && pgx_gl(pair(PGX_TOP + 1, -63)).mant > 0, "the sign of mant is the logarithm's");
    check_value(pair(PGX_TOP, -64), "1/2");
    check_value(pair(PGX_TOP, -65), "1/4");
    // the text: fixed and exponent notation, stripped zeros
    CHECK(text_gl(pgx_gl_of(-1000, 3)) == "-1000" && text_gl(pgx_gl_of(-1200, 1)) == "-12" && text_gl(pgx_gl_of(-1234, 0)) == "-1.234" &&
              text_gl(pgx_gl_of(-3010, -1)) == "-0.301" && text_gl(pgx_gl_of(-1234, -4)) == "-0.0001234" && text_gl(pgx_gl_of(-1230, -5)) == "-1.23e-05" &&
              text_gl(pgx_gl_of(-1000, -12)) == "-1e-12" && text_gl(pgx_gl_of(4709, -20)) == "4.709e-20" && text_gl(pgx_gl_deferred()) == "?",
          "pgx_gl_text");
}

// 200 boundaries t = d.ddd5 10^k: the long double nearest 10^-t is deferred, its neighbours three windows away are decided
static void test_boundaries() {
    int n = 0;
    for (int k = -6; k <= 3 && n < 200; ++k)
        for (int rep = 0; rep < 20; ++rep, ++n) {
            const int d = 1000 + (int)(rnd() % (k == 3 ? 3900 : 9000));   // (t < 4900: above 2^-16300)
            char txt[64];
            snprintf(txt, sizeof txt, "%d5e%d", d, k - 4);                  // d.ddd5 10^k = ddddd5 10^(k - 4)
            const long double t = strtold(txt, nullptr), w = 3.0L * (long double)PG_GL_WINDOW * powl(10.0L, (long double)(k - 3));
            const pgx x = pgx_from_ld(powl(10.0L, -t));
            CHECK(pgx_gl_is_deferred(pgx_gl(x)), "10^-%s is not deferred: \"%s\"", txt, text_gl(pgx_gl(x)).c_str());
            for (int side = -1; side <= 1; side += 2) {
                const pgx y = pgx_from_ld(powl(10.0L, -(t + side * w)));
                const pg_gl g = pgx_gl(y);
                CHECK(!pgx_gl_is_deferred(g), "10^-(%s %+d x 3 windows) is deferred", txt, side);
                if (!pgx_gl_is_deferred(g))
                    CHECK(text_gl(g) == text_ld(pgx_to_ld(y)) && abs((int)g.mant) == d + (side > 0 ? 1 : 0) && g.exp10 == k,
                          "10^-(%s %+d x 3 windows): \"%s\", long double prints \"%s\"", txt, side, text_gl(g).c_str(), text_ld(pgx_to_ld(y)).c_str());
            }
        }
    CHECK(n == 200, "200 boundaries");
}

// ---- records: every GL of random bubbles against a long double std::map restatement of the host route ----
struct Bubble {
    bool kept = true;
    std::vector<uint16_t> id;
    std::vector<uint8_t> pres;
    std::vector<double> m;
    std::vector<int32_t> e;
};
struct Record {
    std::vector<uint16_t> own;
    std::vector<uint16_t> vcf;
    bool has_undefined() const { for (uint16_t x : vcf) if (x == 0xFFFF) return true; return false; }
    unsigned n_defined() const { unsigned n = 0; for (uint16_t x : vcf) n += x != 0xFFFF; return n; }
};

static std::vector<std::string> gl_ld(const Bubble& b, const Record& r, long double* top) {
    typedef std::pair<unsigned, unsigned> G;
    const size_t A = b.id.size();
    std::vector<std::pair<G, long double>> N;
    size_t bin = 0;
    for (size_t x = 0; x < A; ++x)
        for (size_t y = x; y < A; ++y, ++bin)
            if (b.kept && b.pres[x] && b.pres[y]) N.push_back({G(b.id[x], b.id[y]), ldexpl((long double)b.m[bin], b.e[bin])});
    long double sum = 0.0L;
    for (auto& kv : N) sum += kv.second;
    if (sum > 0) for (auto& kv : N) kv.second = kv.second / sum;
    std::map<G, long double> F;                  // Variant::separate_variants
    for (auto& kv : N) {
        unsigned ra = r.own[kv.first.first], rb = r.own[kv.first.second];
        if (ra > rb) std::swap(ra, rb);
        F[G(ra, rb)] += kv.second;
    }
    if (F.empty()) F[G(0, 0)] = 1.0L;
    if (r.has_undefined()) {                     // get_specific_likelihoods over the defined alleles
        std::map<G, long double> S;
        long double sum2 = 0.0L;
        for (auto& kv : F) {
            if (r.vcf[kv.first.first] == 0xFFFF || r.vcf[kv.first.second] == 0xFFFF) continue;
            S[G(r.vcf[kv.first.first], r.vcf[kv.first.second])] += kv.second;
            sum2 += kv.second;
        }
        if (sum2 > 0) for (auto& kv : S) kv.second = kv.second / sum2;
        F.swap(S);
    }
    const unsigned nd = r.n_defined();
    std::vector<long double> all(nd * (nd + 1) / 2, 0.0L);   // get_all_likelihoods
    for (auto& kv : F) all[kv.first.second * (kv.first.second + 1) / 2 + kv.first.first] = kv.second;
    std::vector<std::string> out;
    *top = 0.0L;
    for (long double x : all) { out.push_back(text_ld(x)); if (x > *top) *top = x; }
    return out;
}

struct BubbleKeys {
    const Bubble* b;
    const Record* r;
    size_t x, y, bin;
    void start() { x = 0; y = 0; bin = 0; }
    bool next(pgx* v, uint32_t* key) {
        const size_t A = b->id.size();
        while (x < A) {
            const size_t cx = x, cy = y, cbin = bin;
            ++bin;
            if (++y == A) { ++x; y = x; }
            if (b->kept && b->pres[cx] && b->pres[cy]) {
                uint32_t ra = r->own[b->id[cx]], rb = r->own[b->id[cy]];
                if (ra > rb) std::swap(ra, rb);
                *v = pgx_from_bin(b->m[cbin], b->e[cbin]);
                *key = (ra << 16) | rb;
                return true;
            }
        }
        return false;
    }
};
struct VcfOf {
    const Record* r;
    uint32_t operator()(uint32_t a) const { return r->vcf[a]; }
};
struct Into {
    std::vector<pg_gl>* v;
    void operator()(uint32_t i, pg_gl g) { (*v)[i] = g; }
};

static std::vector<pg_gl> gl_pgx(const Bubble& b, const Record& r) {
    const unsigned nd = r.n_defined();
    std::vector<pg_gl> got(nd * (nd + 1) / 2, pgx_gl_of(7, 7));
    BubbleKeys keys = {&b, &r, 0, 0, 0};
    VcfOf vcf = {&r};
    Into into = {&got};
    pgx_record_gl(keys, (uint32_t)r.vcf.size(), r.has_undefined(), vcf, into);
    return got;
}

static long g_values = 0, g_values_deferred = 0, g_positive = 0;
static void check_record(const Bubble& b, const Record& r, const char* what) {
    long double top;
    const std::vector<std::string> want = gl_ld(b, r, &top);
    const std::vector<pg_gl> got = gl_pgx(b, r);
    CHECK(want.size() == got.size(), "%s: %zu values, %zu expected", what, got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); ++i) {
        ++g_values;
        if (pgx_gl_is_deferred(got[i])) { ++g_values_deferred; continue; }
        if (got[i].mant > 0) ++g_positive;
        CHECK(text_gl(got[i]) == want[i], "%s: A %zu value %zu of %zu: \"%s\", long double prints \"%s\"", what, b.id.size(), i, got.size(),
              text_gl(got[i]).c_str(), want[i].c_str());
    }
}

static double rnd_mant() { return ldexp((double)((rnd() >> 11) | (1ull << 52)), -53); }

static Record rnd_record(unsigned n_ids) {
    Record r;
    const unsigned nA = 1 + rnd() % (n_ids < 6 ? n_ids + 1 : 6);
    r.own.resize(n_ids);
    for (unsigned i = 0; i < n_ids; ++i) r.own[i] = (uint16_t)(i == 0 ? 0 : rnd() % nA);
    r.vcf.resize(nA);
    uint16_t d = 0;
    const bool undef = rnd() % 3 == 0;
    for (unsigned a = 0; a < nA; ++a) r.vcf[a] = (a == 0 || !undef || rnd() % 3) ? d++ : (uint16_t)0xFFFF;
    return r;
}

static void test_records() {
    for (int it = 0; it < 100000; ++it) {
        Bubble b;
        const unsigned A = 1 + rnd() % 8, spread = (rnd() % 4 == 0) ? 401 : (rnd() % 2 ? 8 : 70);
        uint16_t id = 0;
        for (unsigned a = 0; a < A; ++a) { b.id.push_back(id); id += 1 + (rnd() % 5 == 0); b.pres.push_back(rnd() % 6 != 0); }
        b.kept = rnd() % 40 != 0;
        const int32_t base = -(int32_t)(rnd() % 9000);
        for (unsigned k = 0; k < A * (A + 1) / 2; ++k) {
            b.m.push_back(rnd() % 13 == 0 ? 0.0 : rnd_mant());
            b.e.push_back(base - (int32_t)(rnd() % spread));
        }
        const unsigned n_rec = 1 + rnd() % 4;
        for (unsigned q = 0; q < n_rec; ++q) check_record(b, rnd_record(id), "random bubble");
    }
    printf("records: %ld values, %ld deferred, %ld positive\n", g_values, g_values_deferred, g_positive);
    CHECK(g_values > 500000 && (double)g_values_deferred <= 1e-4 * (double)g_values, "the bubbles' values: %ld, %ld deferred", g_values, g_values_deferred);
}

static Bubble bubble3(std::vector<double> m, std::vector<int32_t> e) {
    Bubble b;
    b.id = {0, 1, 2}; b.pres = {1, 1, 1}; b.m = m; b.e = e;
    return b;
}
static Record record(std::vector<uint16_t> own, std::vector<uint16_t> vcf) {
    Record r;
    r.own = own; r.vcf = vcf;
    return r;
}
static bool all_are(const std::vector<pg_gl>& g, const char* text) {
    for (pg_gl x : g) if (text_gl(x) != text) return false;
    return true;
}

static void test_constructed() {
    const std::vector<int32_t> z6(6, 0);
    const double U = 0x1p-64;
    // an empty map: F[(0,0)] = 1
    Bubble nk = bubble3({0.25, 0.375, 0.1875, 0, 0.125, 0.0625}, z6);
    nk.kept = false;
    std::vector<pg_gl> g = gl_pgx(nk, record({0, 1, 0}, {0, 1}));
    CHECK(g.size() == 3 && text_gl(g[0]) == "0" && text_gl(g[1]) == "-inf" && text_gl(g[2]) == "-inf", "an empty map");
    check_record(nk, record({0, 1, 0}, {0, 1}), "an empty map");
    check_record(nk, record({0, 1, 2}, {0, 0xFFFF, 1}), "an empty map, undefined allele");
    // every bin zero
    CHECK(all_are(gl_pgx(bubble3({0, 0, 0, 0, 0, 0}, z6), record({0, 1, 0}, {0, 1})), "-inf"), "every bin zero");
    check_record(bubble3({0, 0, 0, 0, 0, 0}, z6), record({0, 1, 0}, {0, 1}), "every bin zero");
    // a single key, an absent key, a zero bin among the keys
    Bubble one = bubble3({0.7, 0, 0, 0, 0, 0}, z6);
    one.pres = {1, 0, 0};
    g = gl_pgx(one, record({0, 1, 2}, {0, 1, 2}));
    CHECK(g.size() == 6 && text_gl(g[0]) == "0" && all_are(std::vector<pg_gl>(g.begin() + 1, g.end()), "-inf"), "a single key");
    check_record(one, record({0, 1, 2}, {0, 1, 2}), "a single key");
    check_record(bubble3({0.25, 0.5, 0, 0.25, 0, 0}, z6), record({0, 1, 1}, {0, 1, 2}), "an absent key and a zero bin");
    // best = 1 - m 2^-64
    for (int m = 1; m <= 4; ++m) check_record(bubble3({1.0 - 0x1p-53, (2048.0 - m) * U, 0, 0, 0, m * U}, z6), record({0, 0, 1}, {0, 1}), "1 - m 2^-64");
    // defined keys all zero; the likeliest genotype over an undefined allele
    CHECK(all_are(gl_pgx(bubble3({0, 0.5, 0, 0.5, 0, 0}, z6), record({0, 1, 2}, {0, 0xFFFF, 1})), "-inf"), "defined keys all zero");
    check_record(bubble3({0, 0.5, 0, 0.5, 0, 0}, z6), record({0, 1, 2}, {0, 0xFFFF, 1}), "defined keys all zero");
    check_record(bubble3({0.125, 0.5, 0.125, 0, 0, 0.25}, z6), record({0, 1, 2}, {0, 0xFFFF, 1}), "likeliest is undefined");
    // both sides of the cut: the bubble's largest bin, and a folded value
    Bubble lo = bubble3({0.5, 0.75, 0.5, 0.5, 0.5, 0.5}, {-16310, -16301, -16400, -16330, -16305, -16302});
    g = gl_pgx(lo, record({0, 1, 0}, {0, 1}));
    CHECK(g.size() == 3 && pgx_gl_is_deferred(g[0]) && pgx_gl_is_deferred(g[1]) && pgx_gl_is_deferred(g[2]), "largest bin below 2^-16300: all deferred");
    lo.e[1] = -16299;
    g = gl_pgx(lo, record({0, 1, 0}, {0, 1}));
    CHECK(!pgx_gl_is_deferred(g[0]) && !pgx_gl_is_deferred(g[1]), "largest bin at 2^-16300 is decided");
    check_record(lo, record({0, 1, 0}, {0, 1}), "next to the deferral cut");
    g = gl_pgx(bubble3({0.5, 0.5, 0, 0, 0, 0}, {0, -16350, 0, 0, 0, 0}), record({0, 1, 2}, {0, 1, 2}));
    CHECK(text_gl(g[0]) == "0" && pgx_gl_is_deferred(g[1]) && text_gl(g[2]) == "-inf", "a folded value below 2^-16300 is deferred");
}

// a fold whose rounded sum exceeds 1: k quotients onto one key
static void search_above_one() {
    long found = 0;
    for (long it = 0; it < 4000000 && found < 3; ++it) {
        const unsigned n = 2 + rnd() % 5;
        pgx v[6], sum = pgx_zero();
        for (unsigned i = 0; i < n; ++i) { v[i] = pgx_from_bin(rnd_mant(), -(int32_t)(rnd() % 6)); sum = pgx_add(sum, v[i]); }
        pgx f = pgx_zero();
        for (unsigned i = 0; i < n; ++i) f = pgx_add(f, pgx_div(v[i], sum));
        if (pgx_cmp(f, pgx_one()) > 0) {
            ++found;
            printf("above one: %u keys:", n);
            for (unsigned i = 0; i < n; ++i) printf(" (%a, %d)", ldexp((double)v[i].m, -64), v[i].e + 64);
            printf(" -> m %#llx e %d, GL %s\n", (unsigned long long)f.m, f.e, text_gl(pgx_gl(f)).c_str());
        }
    }
    printf("search: %ld folds above one\n", found);
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 10000000L;
    test_constants();
    test_special();
    test_boundaries();
    test_random(n);
    test_records();
    test_constructed();
    if (argc > 2 && !strcmp(argv[2], "search")) search_above_one();
    printf("%ld checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
