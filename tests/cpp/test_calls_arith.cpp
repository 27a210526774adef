// test_calls_arith.cpp — the integer-pair arithmetic of the device's genotype calls (pangenie_amd/csrc/pg_calls.h)
// against this machine's x87 long double, bit for bit.  Stand-alone: g++ -std=c++17 -I pangenie_amd/csrc, no device.
//
// What the kernels decide with these functions the reference decides in long double (src/genotypingresult.cpp:118-210),
// so every function has to give the very bits the FPU gives: add, sub, div, compare, the conversion of a bin, 1 - x next
// to 1, the genotype-quality table against (size_t)(-10 log10l(x)), and the whole decision against a long double
// restatement of normalize / get_likeliest_genotype / get_genotype_quality.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pg_calls.h"

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

static bool same(pgx a, long double x) {
    const pgx b = pgx_from_ld(x);
    return a.m == b.m && (a.m == 0 || a.e == b.e);
}

// a random operand: a full 64-bit mantissa, one with 53 bits (what a bin carries), or one with long runs of zeros and ones
static pgx rnd_operand(int e_lo, int e_hi) {
    pgx r;
    const uint64_t kind = rnd() % 4;
    uint64_t m = rnd();
    if (kind == 1) m &= ~0x7FFull;
    if (kind == 2) m = (rnd() & 1) ? (m | (~0ull >> (rnd() % 64))) : (m & (~0ull << (rnd() % 64)));
    if (kind == 3) m = (m & (~0ull << (rnd() % 64))) | (1ull << (rnd() % 64));
    r.m = m | PGX_TOP;
    r.e = e_lo + (int)(rnd() % (uint64_t)(e_hi - e_lo + 1));
    return r;
}

static void check_pair(pgx a, pgx b) {
    const long double x = pgx_to_ld(a), y = pgx_to_ld(b);
    CHECK(same(pgx_from_ld(x), x) && pgx_from_ld(x).m == a.m, "round trip");
    CHECK(same(pgx_add(a, b), x + y), "add m=%016llx e=%d + m=%016llx e=%d", (unsigned long long)a.m, a.e, (unsigned long long)b.m, b.e);
    CHECK(same(pgx_add(b, a), y + x), "add (swapped)");
    const int c = pgx_cmp(a, b);
    CHECK(c == (x < y ? -1 : (x > y ? 1 : 0)), "cmp");
    if (c >= 0) CHECK(same(pgx_sub(a, b), x - y), "sub m=%016llx e=%d - m=%016llx e=%d", (unsigned long long)a.m, a.e, (unsigned long long)b.m, b.e);
    else CHECK(same(pgx_sub(b, a), y - x), "sub m=%016llx e=%d - m=%016llx e=%d", (unsigned long long)b.m, b.e, (unsigned long long)a.m, a.e);
    CHECK(same(pgx_div(a, b), x / y), "div m=%016llx e=%d / m=%016llx e=%d", (unsigned long long)a.m, a.e, (unsigned long long)b.m, b.e);
    CHECK(same(pgx_div(b, a), y / x), "div (swapped)");
}

static void test_random_pairs() {
    for (int i = 0; i < 1000000; ++i) {
        pgx a = rnd_operand(-300, 300), b;
        const uint64_t k = rnd() % 8;
        if (k < 5) {   // every exponent gap 0 .. 70 in turn, either sign
            b = rnd_operand(0, 0);
            b.e = a.e + ((rnd() & 1) ? 1 : -1) * (int)(i % 71);
        } else if (k == 5) {   // and beyond: 71 .. 400
            b = rnd_operand(0, 0);
            b.e = a.e - 71 - (int)(rnd() % 330);
        } else if (k == 6) {   // nearly equal: cancellation
            b = a;
            b.m = (a.m ^ (rnd() & ((1ull << (rnd() % 40)) - 1))) | PGX_TOP;
        } else b = rnd_operand(-300, 300);
        check_pair(a, b);
    }
}

static void test_ties_and_carries() {
    // a + half an ulp of a: a tie, to the even neighbour; with anything below the half: up
    for (int i = 0; i < 20000; ++i) {
        pgx a = rnd_operand(-50, 50);
        pgx h; h.m = PGX_TOP; h.e = a.e - 64;          // = 2^(a.e - 1)
        CHECK(same(pgx_add(a, h), pgx_to_ld(a) + pgx_to_ld(h)), "tie add");
        pgx h3 = h; h3.m = PGX_TOP | (1ull << (rnd() % 63));   // just above the half
        CHECK(same(pgx_add(a, h3), pgx_to_ld(a) + pgx_to_ld(h3)), "above tie add");
        pgx q; q.m = ~0ull; q.e = a.e - 65;           // just below the half
        CHECK(same(pgx_add(a, q), pgx_to_ld(a) + pgx_to_ld(q)), "below tie add");
        // a - half an ulp of the RESULT's binade, and a sticky bit far below it
        CHECK(same(pgx_sub(a, h), pgx_to_ld(a) - pgx_to_ld(h)), "tie sub");
        pgx t; t.m = PGX_TOP | rnd(); t.e = a.e - 64 - 1 - (int)(rnd() % 130);
        CHECK(same(pgx_sub(a, t), pgx_to_ld(a) - pgx_to_ld(t)), "sticky sub");
        CHECK(same(pgx_add(a, t), pgx_to_ld(a) + pgx_to_ld(t)), "sticky add");
        pgx p2; p2.m = PGX_TOP; p2.e = a.e;           // a power of two minus something tiny: the result changes binade
        CHECK(same(pgx_sub(p2, t), pgx_to_ld(p2) - pgx_to_ld(t)), "power of two minus tiny");
        CHECK(same(pgx_sub(p2, h), pgx_to_ld(p2) - pgx_to_ld(h)), "power of two minus half ulp");
    }
    // the carry out of rounding: all ones + half an ulp -> the next power of two
    pgx ones; ones.m = ~0ull; ones.e = -3;
    pgx h; h.m = PGX_TOP; h.e = ones.e - 64;
    pgx s = pgx_add(ones, h);
    CHECK(s.m == PGX_TOP && s.e == ones.e + 1, "carry out of rounding (add)");
    CHECK(same(s, pgx_to_ld(ones) + pgx_to_ld(h)), "carry out of rounding (add) against the FPU");
    // the carry out of the addition itself, then a tie
    pgx b = ones;
    CHECK(same(pgx_add(ones, b), pgx_to_ld(ones) + pgx_to_ld(b)), "carry out of the addition");
    pgx one_ulp; one_ulp.m = PGX_TOP; one_ulp.e = ones.e - 63;
    CHECK(same(pgx_add(ones, one_ulp), pgx_to_ld(ones) + pgx_to_ld(one_ulp)), "all ones + one ulp");
    // division: a quotient that rounds up into the next binade, and exact quotients
    for (int i = 0; i < 20000; ++i) {
        pgx d = rnd_operand(-20, 20);
        pgx n = d; n.m = d.m - 1 - (rnd() % 3); n.m |= PGX_TOP;
        CHECK(same(pgx_div(n, d), pgx_to_ld(n) / pgx_to_ld(d)), "div just below one");
        CHECK(same(pgx_div(d, n), pgx_to_ld(d) / pgx_to_ld(n)), "div just above one");
        CHECK(same(pgx_div(d, d), 1.0L), "x / x");
        pgx small; small.m = (uint64_t)(1 + rnd() % 1000) << 32; small.m <<= __builtin_clzll(small.m); small.e = -70;
        CHECK(same(pgx_div(d, small), pgx_to_ld(d) / pgx_to_ld(small)), "div by a short mantissa");
    }
    // zeros
    const pgx z = pgx_zero(), a = rnd_operand(0, 0);
    CHECK(same(pgx_add(z, a), pgx_to_ld(a)) && same(pgx_add(a, z), pgx_to_ld(a)) && same(pgx_add(z, z), 0.0L), "add zero");
    CHECK(same(pgx_sub(a, z), pgx_to_ld(a)) && same(pgx_sub(a, a), 0.0L), "sub zero");
    CHECK(same(pgx_div(z, a), 0.0L), "zero / x");
    CHECK(pgx_cmp(z, a) == -1 && pgx_cmp(a, z) == 1 && pgx_cmp(z, z) == 0, "cmp zero");
}

static void test_conversion() {
    for (int i = 0; i < 200000; ++i) {
        const double m = ldexp((double)((rnd() >> 11) | (1ull << 52)), -53);   // [0.5, 1)
        const int32_t e = (int32_t)(rnd() % 32500) - 16500;   // down past the flush to zero, up to 2^16000
        const long double want = ldexpl((long double)m, e);
        const pgx got = pgx_from_bin(m, e);
        if (want == 0.0L || want >= ldexpl(1.0L, -16382)) CHECK(same(got, want), "bin %a * 2^%d", m, e);
        else CHECK(got.m != 0, "a bin that is a subnormal long double reads as 0");   // subnormal: only zero-or-not is modelled
    }
    CHECK(pgx_from_bin(0.0, 5).m == 0 && pgx_from_bin(-0.5, 5).m == 0, "zero and negative bins");
    // the edge of ldexpl's flush to zero: 2^-16446 is 0 (a tie to even), the next double above it is not
    CHECK(ldexpl(0.5L, -16445) == 0.0L && pgx_from_bin(0.5, -16445).m == 0, "2^-16446 reads 0");
    CHECK(ldexpl((long double)nextafter(0.5, 1.0), -16445) > 0.0L && pgx_from_bin(nextafter(0.5, 1.0), -16445).m != 0, "just above 2^-16446 does not");
    CHECK(pgx_from_bin(nextafter(1.0, 0.0), -16446).m == 0 && ldexpl((long double)nextafter(1.0, 0.0), -16446) == 0.0L, "just below 2^-16446 reads 0");
    // general doubles (the tie threshold is one), subnormal doubles included
    CHECK(same(pgx_tie_threshold(), (long double)0.0000000001), "tie threshold is the widened double literal");
    CHECK(!same(pgx_tie_threshold(), 0.0000000001L), "... and not the long double literal");
    CHECK(same(pgx_from_double(5e-324, 0), (long double)5e-324) && same(pgx_from_double(3e-310, 7), ldexpl((long double)3e-310, 7)), "subnormal doubles");
    CHECK(same(pgx_from_double(1.0, 0), 1.0L) && same(pgx_one(), 1.0L), "one");
    // the deferral cut
    CHECK(pgx_below_pow2(pgx_from_bin(nextafter(1.0, 0.0), -16300), -16300) && !pgx_below_pow2(pgx_from_bin(0.5, -16299), -16300), "2^-16300 cut");
}

static void test_one_minus() {
    for (int j = 0; j <= 64; ++j) {
        const long double x = 1.0L - (long double)j * ldexpl(1.0L, -64);
        CHECK(same(pgx_one_minus(pgx_from_ld(x)), 1.0L - x), "1 - (1 - %d 2^-64)", j);
    }
    for (int i = 0; i < 100000; ++i) {
        pgx x = rnd_operand(-64 - (int)(rnd() % 80), -64);   // anything in (0, 1)
        CHECK(same(pgx_one_minus(x), 1.0L - pgx_to_ld(x)), "1 - x");
    }
    CHECK(pgx_one_minus(pgx_one()).m == 0, "1 - 1");
}

static std::vector<uint64_t> g_tm(PG_GQ_STEPS);
static std::vector<int32_t> g_te(PG_GQ_STEPS);

static void check_gq(long double x) {
    if (!(x > 0.0L) || x > 1.0L) return;
    CHECK(pgx_gq(pgx_from_ld(x), g_tm.data(), g_te.data()) == (uint32_t)pgx_gq_host(x), "gq of %.25Lg: %u, host %zu", x,
          pgx_gq(pgx_from_ld(x), g_tm.data(), g_te.data()), pgx_gq_host(x));
}

static void test_gq_table() {
    CHECK(pgx_build_gq_table(g_tm.data(), g_te.data()) == 0, "the table search ended");
    CHECK(g_tm[0] == PGX_TOP && g_te[0] == -63, "entry 0 is 1");
    for (int k = 1; k < PG_GQ_STEPS; ++k) {
        pgx a, b;
        a.m = g_tm[k - 1]; a.e = g_te[k - 1]; b.m = g_tm[k]; b.e = g_te[k];
        CHECK(pgx_cmp(b, a) < 0, "table is strictly descending at %d", k);
        const long double t = pgx_to_ld(b);
        CHECK(pgx_gq_host(t) >= (size_t)k && pgx_gq_host(nextafterl(t, 2.0L)) < (size_t)k, "entry %d is the largest x of its class", k);
        long double lo = t, hi = t;
        for (int s = 0; s < 40; ++s) {   // both sides of every threshold
            check_gq(lo); check_gq(hi);
            lo = nextafterl(lo, 0.0L); hi = nextafterl(hi, 2.0L);
        }
        check_gq(powl(10.0L, -(long double)k / 10.0L));
    }
    for (int m = 1; m <= 5000; ++m) check_gq((long double)m * ldexpl(1.0L, -64));
    CHECK(pgx_gq(pgx_from_ld(ldexpl(1.0L, -64)), g_tm.data(), g_te.data()) == 192, "2^-64 gives 192");
    CHECK(pgx_gq(pgx_zero(), g_tm.data(), g_te.data()) == PG_GQ_CERTAIN, "0 gives 10000");
    check_gq(1.0L);
    for (int i = 0; i < 200000; ++i) check_gq(pgx_to_ld(rnd_operand(-127, -64)));   // [2^-64, 1): what 1 - best can be
}

// ---- the whole decision against a long double restatement of the reference ----
struct VecKeys {
    const std::vector<double>* m;
    const std::vector<int32_t>* e;
    size_t i;
    void start() { i = 0; }
    bool next(pgx* v) {
        if (i >= m->size()) return false;
        *v = pgx_from_bin((*m)[i], (*e)[i]);
        ++i;
        return true;
    }
};

static pgx_decision decide_ld(const std::vector<long double>& bins) {
    pgx_decision r = {PGX_CALL_NONE, 0, 0};
    if (bins.empty()) return r;
    std::vector<long double> v = bins;
    long double sum = 0.0L;
    for (long double x : v) sum += x;                      // normalize
    if (sum > 0) for (long double& x : v) x = x / sum;
    long double best = 0.0L;
    size_t bi = 0;
    for (size_t i = 0; i < v.size(); ++i) if (v[i] >= best) { best = v[i]; bi = i; }   // get_likeliest_genotype
    bool unique = true;
    for (size_t i = 0; i < v.size(); ++i) if (i != bi && fabsl(v[i] - best) < 0.0000000001) unique = false;
    if (!(best > 0.0L)) return r;
    if (!unique) { r.flags = PGX_CALL_NOT_UNIQUE; return r; }
    r.flags = PGX_CALL_OK;
    r.best = (uint32_t)bi;
    const long double pw = 1.0L - best;                    // get_genotype_quality
    r.gq = pw > 0.0 ? (uint32_t)(size_t)(-10 * log10l(pw)) : 10000u;
    return r;
}

static void check_variant(const std::vector<double>& m, const std::vector<int32_t>& e, const char* what) {
    std::vector<long double> ld(m.size());
    for (size_t i = 0; i < m.size(); ++i) ld[i] = ldexpl((long double)m[i], e[i]);
    VecKeys keys = {&m, &e, 0};
    const pgx_decision got = pgx_decide(keys, g_tm.data(), g_te.data());
    const pgx_decision want = decide_ld(ld);
    CHECK(got.flags == want.flags && (got.flags != PGX_CALL_OK || (got.best == want.best && got.gq == want.gq)),
          "%s: %zu bins: flags %u best %u gq %u, long double: flags %u best %u gq %u", what, m.size(), got.flags, got.best, got.gq, want.flags,
          want.best, want.gq);
}

static double rnd_mant() { return ldexp((double)((rnd() >> 11) | (1ull << 52)), -53); }

static void test_decisions() {
    for (int it = 0; it < 200000; ++it) {
        const size_t n = 1 + rnd() % 15;
        std::vector<double> m(n);
        std::vector<int32_t> e(n);
        const int32_t base = -(int32_t)(rnd() % 16000);
        const uint64_t style = rnd() % 6;
        for (size_t i = 0; i < n; ++i) {
            m[i] = rnd_mant();
            e[i] = base - (int32_t)(rnd() % (style == 0 ? 4 : (style == 1 ? 40 : (style == 2 ? 80 : 300))));
            if (rnd() % 11 == 0) m[i] = 0.0;
        }
        if (style == 4 && n > 1) { const size_t j = rnd() % n, k = rnd() % n; m[k] = m[j]; e[k] = e[j]; }   // equal maxima, perhaps
        if (style == 5) e[rnd() % n] = base + 70 + (int32_t)(rnd() % 200);   // one bin that owns the sum: GQ near the top
        check_variant(m, e, "random");
    }
    // a runner-up on both sides of the tie threshold: best = 0.5 (1 + t), second = 0.5 (1 - t), difference t
    for (int s = -40; s <= 40; ++s) {
        const double t = 1e-10 * (1.0 + s * ldexp(1.0, -24));
        std::vector<double> m = {0.5 * (1.0 - t), 0.5 * (1.0 + t)};
        std::vector<int32_t> e = {-700, -700};
        check_variant(m, e, "tie threshold");
    }
    check_variant({}, {}, "no keys");
    check_variant({0.0, 0.0, 0.0}, {0, 0, 0}, "all zero");
    check_variant({0.75}, {-90}, "one key");
    check_variant({0.0}, {0}, "one zero key");
    // deferred, and only there
    VecKeys k1;
    std::vector<double> m = {0.5, 0.75, 0.5};
    std::vector<int32_t> e = {-16310, -16301, -16400};
    k1 = {&m, &e, 0};
    CHECK(pgx_decide(k1, g_tm.data(), g_te.data()).flags == PGX_CALL_DEFERRED, "largest bin below 2^-16300 is deferred");
    e[1] = -16299;
    k1 = {&m, &e, 0};
    CHECK(pgx_decide(k1, g_tm.data(), g_te.data()).flags != PGX_CALL_DEFERRED, "largest bin at 2^-16300 is decided");
    check_variant(m, e, "next to the deferral cut");
    check_variant({0.5, 0.75, 0.5, 0.9}, {-16250, -16299, -16500, -16440}, "small bins beside a decided one");
}

int main() {
    test_random_pairs();
    test_ties_and_carries();
    test_conversion();
    test_one_minus();
    test_gq_table();
    test_decisions();
    printf("%ld checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
