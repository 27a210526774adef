// test_combine_arith.cpp — the arithmetic of the path-subset flow on the device (pangenie_amd/csrc/pg_combine.h) against
// this machine's x87 long double, bit for bit.  Stand-alone: g++ -std=c++17 -I pangenie_amd/csrc, no device.
//
// What k_combine does per genotype key the reference does with GenotypingResult::combine, `map[key] += value` in long
// double over the path subsets (src/genotypingresult.cpp:193-198), and what k_ccalls decides the reference decides on the
// combined map (src/genotypingresult.cpp:118-210).  Checked here: a summand as ldexpl reads it (subnormal results
// included), the fold of one key in the caller's order, the deferral rule, and the walker over combined bins with
// pgx_decide against a long double restatement.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pg_combine.h"

static_assert(LDBL_MANT_DIG == 64, "this test needs the x87 80-bit long double");
static_assert(sizeof(pg_combined_bin) == 16, "a combined bin is 16 bytes");

static int g_fail = 0;
static long g_checks = 0;
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

static bool same(pgx a, long double x) {
    const pgx b = pgx_from_ld(x);
    return a.m == b.m && (a.m == 0 || a.e == b.e);
}
static bool bin_is(pg_combined_bin b, long double x) {
    pgx v;
    v.m = b.m;
    v.e = b.e;
    return b.flags == PG_COMBINED_PRESENT && (b.m != 0 || b.e == 0) && same(v, x) && ldexpl((long double)b.m, b.e) == x;
}

// a mantissa in [0.5, 1) with 53 random bits, with few bits, or with its last bit set
static double rnd_mant() {
    uint64_t f = rnd() >> 11;
    const uint64_t kind = rnd() % 4;
    if (kind == 1) f &= ~0ull << (rnd() % 52);
    if (kind == 2) f |= 1ull;
    return ldexp((double)(f | (1ull << 52)), -53);
}

struct Summand {
    bool held;
    double lik;
    int32_t lik_exp;
};

// the device's fold and the host's, over the chains that hold the key
static pg_combined_bin fold_of(const std::vector<Summand>& s) {
    pgc_fold f;
    pgc_fold_init(&f);
    for (const Summand& x : s)
        if (x.held) pgc_fold_take(&f, pgc_summand(x.lik, x.lik_exp));
    return pgc_fold_bin(&f);
}
struct HostKey {
    bool present;
    long double value, largest;
};
static HostKey host_of(const std::vector<Summand>& s) {
    HostKey h = {false, 0.0L, 0.0L};
    for (const Summand& x : s) {
        if (!x.held) continue;
        const long double v = ldexpl((long double)x.lik, x.lik_exp);   // the bin as the host reads it
        h.value = h.present ? h.value + v : 0.0L + v;                   // map[key] += value
        h.present = true;
        if (v > h.largest) h.largest = v;
    }
    return h;
}

static void check_key(const std::vector<Summand>& s, const char* what) {
    const pg_combined_bin b = fold_of(s);
    const HostKey h = host_of(s);
    const bool cut = h.largest > 0.0L && h.largest < ldexpl(1.0L, PG_CALLS_DEFER_EXP);
    if (!h.present) { CHECK(b.flags == 0 && b.m == 0 && b.e == 0, "%s: a key no chain holds is absent", what); return; }
    CHECK(((b.flags & PG_COMBINED_DEFERRED) != 0) == cut, "%s: deferred %u, largest summand below the cut %d", what, b.flags, (int)cut);
    if (b.flags & PG_COMBINED_DEFERRED) { CHECK(b.flags == (PG_COMBINED_PRESENT | PG_COMBINED_DEFERRED) && b.m == 0 && b.e == 0, "%s: a deferred bin carries no value", what); return; }
    CHECK(bin_is(b, h.value), "%s: %zu summands: m=%016llx e=%d, long double %La", what, s.size(), (unsigned long long)b.m, b.e, h.value);
}

static void test_summand() {
    for (int i = 0; i < 300000; ++i) {   // around and inside the subnormal range, and far from it
        const double m = (i % 7 == 0) ? 0.5 : rnd_mant();
        const int32_t e = (i % 3 == 0) ? -(int32_t)(rnd() % 400) : -16300 - (int32_t)(rnd() % 200);
        CHECK(same(pgc_summand(m, e), ldexpl((long double)m, e)), "summand %a 2^%d", m, e);
    }
    // halves of the quantum: ties to even, and just beside them
    for (int q = 0; q < 64; ++q)
        for (int d = -1; d <= 1; ++d) {
            const double m = ldexp((double)(2 * q + 1) + d * ldexp(1.0, -40), -8);   // (q + 1/2) quanta, a hair less, a hair more
            CHECK(same(pgc_summand(m, PGC_LD_QUANTUM_EXP + 7), ldexpl((long double)m, PGC_LD_QUANTUM_EXP + 7)), "half a quantum %d %d", q, d);
        }
    CHECK(pgc_summand(0.5, PG_CALLS_ZERO_EXP + 1).m == 0, "half the smallest subnormal reads 0");
    CHECK(pgc_summand(0.75, PG_CALLS_ZERO_EXP + 1).m == PGX_TOP && pgc_summand(0.75, PG_CALLS_ZERO_EXP + 1).e == PGC_LD_QUANTUM_EXP - 63, "above it reads the smallest subnormal");
    CHECK(pgc_summand(0.0, 5).m == 0 && pgc_summand(-1.0, 5).m == 0, "zero and negative bins read 0");
}

static void test_random_keys() {
    for (int it = 0; it < 1000000; ++it) {
        const size_t S = 1 + rnd() % 8;
        std::vector<Summand> s(S);
        const int32_t base = 300 - (int32_t)(rnd() % 600);
        for (size_t i = 0; i < S; ++i) {
            s[i].held = rnd() % 5 != 0;
            s[i].lik = rnd() % 9 == 0 ? 0.0 : rnd_mant();
            s[i].lik_exp = base - (int32_t)((it + 17 * i) % 131);   // exponent gaps 0 .. 130, all of them in turn
        }
        check_key(s, "random");
    }
}

static void test_widths() {
    // operand pairs whose exact sum needs 54 .. 64 bits (kept exactly) and 65 bits (the last bit is the half bit: a tie)
    for (int gap = 1; gap <= 12; ++gap)
        for (int it = 0; it < 4000; ++it) {
            uint64_t fa = (rnd() >> 11) | (1ull << 52) | 1ull, fb = (rnd() >> 11) | (1ull << 52) | 1ull;   // 53 bits, the last one set
            if (it % 2) { fa &= ~(1ull << 51); fb &= ~(1ull << 51); }   // both below 0.75: no carry out of the sum
            const Summand a = {true, ldexp((double)fa, -53), 40}, b = {true, ldexp((double)fb, -53), 40 - gap};
            const long double exact_hi = ldexpl((long double)a.lik, a.lik_exp), exact_lo = ldexpl((long double)b.lik, b.lik_exp);
            const long double sum = exact_hi + exact_lo;
            if (gap <= 10) CHECK(sum - exact_hi == exact_lo, "a %d-bit sum is exact", 53 + gap);
            check_key({a, b}, "width");
            check_key({b, a}, "width, swapped");
            check_key({a, b, b}, "width, three");
        }
}

static void test_order() {
    const Summand one = {true, 0.5, 1}, t = {true, 0.5, -63};   // 1 and 2^-64
    const pg_combined_bin x = fold_of({one, t, t}), y = fold_of({t, t, one});
    CHECK(bin_is(x, 1.0L), "(1 + 2^-64) + 2^-64 == 1");
    CHECK(bin_is(y, 1.0L + ldexpl(1.0L, -63)), "(2^-64 + 2^-64) + 1 == 1 + 2^-63");
    CHECK((1.0L + ldexpl(1.0L, -64)) + ldexpl(1.0L, -64) == 1.0L && (ldexpl(1.0L, -64) + ldexpl(1.0L, -64)) + 1.0L == 1.0L + ldexpl(1.0L, -63), "the x87 agrees");
    check_key({one, t, t}, "order a");
    check_key({t, t, one}, "order b");
    // absent chains do not count, a chain that holds the key with 0 makes it present
    const Summand absent = {false, 0.75, 3}, zero = {true, 0.0, 0};
    CHECK(fold_of({absent, absent}).flags == 0, "no chain holds it");
    CHECK(bin_is(fold_of({absent, zero, absent}), 0.0L), "held with the value 0: present and 0");
    CHECK(bin_is(fold_of({absent, one}), 1.0L), "one chain alone: its own value");
}

static void test_deferral() {
    for (int it = 0; it < 400000; ++it) {
        const size_t S = 1 + rnd() % 8;
        std::vector<Summand> s(S);
        const uint64_t style = rnd() % 4;
        for (size_t i = 0; i < S; ++i) {
            s[i].held = rnd() % 6 != 0;
            s[i].lik = rnd() % 10 == 0 ? 0.0 : rnd_mant();
            if (style == 0) s[i].lik_exp = -16200 - (int32_t)(rnd() % 300);          // both sides of the cut and of the subnormals
            else if (style == 1) s[i].lik_exp = -16290 - (int32_t)(rnd() % 20);      // at the cut
            else if (style == 2) s[i].lik_exp = -16360 - (int32_t)(rnd() % 100);     // subnormal and nearly so: all of them deferred
            else s[i].lik_exp = (rnd() & 1) ? -16299 + (int32_t)(rnd() % 3) - (int32_t)(rnd() % 70) * (int32_t)(rnd() & 1) : -16380 - (int32_t)(rnd() % 70);
        }
        check_key(s, "next to the subnormals");
    }
    // a tiny summand beside a large one, in front of it and behind it: not deferred, the x87's sum
    for (int it = 0; it < 50000; ++it) {
        const Summand big = {true, rnd_mant(), -(int32_t)(rnd() % 16299)}, tiny = {true, rnd_mant(), -16383 - (int32_t)(rnd() % 70)};
        const Summand mid = {true, rnd_mant(), big.lik_exp - 60 - (int32_t)(rnd() % 10)};
        CHECK(!(fold_of({tiny, big}).flags & PG_COMBINED_DEFERRED), "a large summand keeps the key on the device");
        check_key({tiny, big}, "tiny, large");
        check_key({big, tiny}, "large, tiny");
        check_key({mid, tiny, big}, "mid, tiny, large");
        check_key({tiny, tiny, mid, big, tiny}, "tiny, tiny, mid, large, tiny");
    }
    // the example of pg_combine.h: the rounding of tiny as the host reads it reaches the half bit of large through mid
    const Summand large = {true, 0.5, -16299}, mid = {true, 0.5, -16363}, tiny = {true, 0.5 + ldexp(1.0, -21), -16427};
    check_key({mid, tiny, large}, "mid + tiny + large");
    pgx with53 = pgx_add(pgx_add(pgx_from_bin(mid.lik, mid.lik_exp), pgx_from_bin(tiny.lik, tiny.lik_exp)), pgx_from_bin(large.lik, large.lik_exp));
    CHECK(!same(with53, host_of({mid, tiny, large}).value), "with all 53 bits of the tiny summand the sum is another: the cut alone would not do");
    CHECK(bin_is(fold_of({mid, tiny, large}), ldexpl(1.0L, -16300)), "both ties stay");
}

// ---- the walker and pgx_decide on combined bins against a long double restatement of the reference ----
static std::vector<uint64_t> g_tm(PG_GQ_STEPS);
static std::vector<int32_t> g_te(PG_GQ_STEPS);

static pgx_decision decide_ld(const std::vector<long double>& bins) {
    pgx_decision r = {PGX_CALL_NONE, 0, 0};
    if (bins.empty()) return r;
    std::vector<long double> v = bins;
    long double sum = 0.0L, largest = 0.0L;
    for (long double x : v) { sum += x; if (x > largest) largest = x; }   // normalize
    if (sum > 0 && largest < ldexpl(1.0L, PG_CALLS_DEFER_EXP)) { r.flags = PGX_CALL_DEFERRED; return r; }
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

static void test_walker() {
    CHECK(pgx_build_gq_table(g_tm.data(), g_te.data()) == 0, "the table search ended");
    for (int it = 0; it < 200000; ++it) {
        const uint32_t A = 1 + (uint32_t)(rnd() % 6), n = A * (A + 1) / 2;
        std::vector<pg_combined_bin> bins(n);
        std::vector<long double> ld;
        std::vector<uint32_t> bin_of_key;
        bool any_deferred = false;
        const int32_t base = -(int32_t)(rnd() % 16000);
        const uint64_t style = rnd() % 5;
        for (uint32_t i = 0; i < n; ++i) {
            // each bin the fold of one to three chains, as k_combine leaves it
            std::vector<Summand> s(1 + rnd() % 3);
            for (Summand& x : s) {
                x.held = rnd() % 4 != 0;
                x.lik = rnd() % 9 == 0 ? 0.0 : rnd_mant();
                x.lik_exp = base - (int32_t)(rnd() % (style == 0 ? 3 : (style == 1 ? 40 : 200)));
                if (style == 4 && rnd() % 40 == 0) x.lik_exp = -16300 - (int32_t)(rnd() % 100);
            }
            bins[i] = fold_of(s);
            if (style == 3 && i && rnd() % 3 == 0) bins[i] = bins[rnd() % i];   // equal maxima, perhaps
            if (!(bins[i].flags & PG_COMBINED_PRESENT)) continue;
            if (bins[i].flags & PG_COMBINED_DEFERRED) any_deferred = true;
            ld.push_back(ldexpl((long double)bins[i].m, bins[i].e));
            bin_of_key.push_back(i);
        }
        pgc_keys keys;
        keys.bins = bins.data();
        keys.n = n;
        keys.i = 0;
        keys.deferred = false;
        const pgx_decision got = pgx_decide(keys, g_tm.data(), g_te.data());
        CHECK(keys.deferred == any_deferred, "a deferred bin is seen");
        if (any_deferred) continue;
        const pgx_decision want = decide_ld(ld);
        CHECK(got.flags == want.flags && (got.flags != PGX_CALL_OK || (got.best == want.best && got.gq == want.gq)),
              "walker: %u bins: flags %u best %u gq %u, long double: flags %u best %u gq %u", n, got.flags, got.best, got.gq, want.flags, want.best, want.gq);
        if (got.flags == PGX_CALL_OK) {
            const uint32_t bin = keys.bin_of(got.best);
            uint32_t sa, sb;
            pgc_slots_of_bin(A, bin, &sa, &sb);
            CHECK(bin == bin_of_key[want.best] && sa <= sb && sb < A && sa * A - sa * (sa - 1) / 2 + (sb - sa) == bin, "the best key's bin and slots");
        }
    }
    // the union of {0, 1} and {0, 2}: five keys, (1, 2) is none of them
    std::vector<pg_combined_bin> u(6);
    const Summand x = {true, 0.75, -20}, no = {false, 0.0, 0};
    const bool in01[6] = {true, true, false, true, false, false}, in02[6] = {true, false, true, false, false, true};
    for (int i = 0; i < 6; ++i) u[i] = fold_of({in01[i] ? x : no, in02[i] ? x : no});
    pgc_keys keys = {u.data(), 6, 0, false};
    pgx v;
    uint32_t seen = 0;
    keys.start();
    while (keys.next(&v)) ++seen;
    CHECK(seen == 5 && u[4].flags == 0, "the union of the key sets is no product of allele masks");
}

int main() {
    test_summand();
    test_random_keys();
    test_widths();
    test_order();
    test_deferral();
    test_walker();
    printf("%ld checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
