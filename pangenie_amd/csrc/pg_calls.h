// pg_calls.h — the arithmetic of the genotype calls (GT, GQ) formed on the device: pg_calls.hip, DESIGN.md §4e.
//
// The reference takes these decisions in x87 `long double` (64-bit mantissa, round to nearest even): normalisation
// (src/genotypingresult.cpp:200-210), likeliest genotype (:149-180), genotype quality (:118-137).  fp64 cannot repeat
// them, so a value here is an integer pair
//     x = m * 2^e,   m in [2^63, 2^64) or m == 0 (then e == 0)
// and every operation rounds its exact result to 64 bits, ties to even — which is what the x87 does as long as the
// value stays a NORMAL long double (exponent >= -16382).  The caller keeps variants near that limit away (PG_CALL_DEFERRED).
//
// Host and device: the same functions compile into the kernels and into tests/cpp/test_calls_arith.cpp, which checks
// every one of them against the machine's long double, bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define PGX_FN __host__ __device__ static inline
#else
#define PGX_FN static inline
#endif

struct pgx {
    uint64_t m;
    int32_t e;
};

#define PGX_TOP 0x8000000000000000ull
#define PG_GQ_STEPS 193        // thresholds k = 0 .. 192: 2^-64, the smallest 1 - best, gives 192.66
#define PG_GQ_CERTAIN 10000    // 1 - best == 0 (reference src/genotypingresult.cpp:136)
// A variant whose largest bin lies below 2^PG_CALLS_DEFER_EXP is not decided on the device: long double has
// subnormals below 2^-16382, which the pair does not model.
#define PG_CALLS_DEFER_EXP (-16300)
// ldexpl() answers 0 for a bin at or below half of the smallest subnormal, 2^-16446 (ties to even): so does pgx_from_bin
#define PG_CALLS_ZERO_EXP (-16446)

PGX_FN pgx pgx_zero() { pgx r; r.m = 0; r.e = 0; return r; }
PGX_FN pgx pgx_one() { pgx r; r.m = PGX_TOP; r.e = -63; return r; }
PGX_FN bool pgx_is_zero(pgx a) { return a.m == 0; }

// -1 / 0 / 1 for a < / == / > b (both non-negative, normalised)
PGX_FN int pgx_cmp(pgx a, pgx b) {
    if (a.m == 0 || b.m == 0) return a.m == b.m ? 0 : (a.m == 0 ? -1 : 1);
    if (a.e != b.e) return a.e < b.e ? -1 : 1;
    return a.m == b.m ? 0 : (a.m < b.m ? -1 : 1);
}

// exact: d * 2^ex for a finite d >= 0 (53 bits fit the mantissa); negative, NaN and infinite d read as 0
PGX_FN pgx pgx_from_double(double d, int32_t ex) {
    union { double f; uint64_t u; } c;
    c.f = d;
    const uint64_t frac = c.u & 0x000FFFFFFFFFFFFFull;
    const int32_t be = (int32_t)((c.u >> 52) & 0x7FFu);
    if ((c.u >> 63) || be == 0x7FF) return pgx_zero();
    uint64_t m;
    int32_t e;
    if (be == 0) {  // subnormal double: frac * 2^-1074
        if (frac == 0) return pgx_zero();
        const int s = __builtin_clzll(frac);
        m = frac << s;
        e = -1074 - s;
    } else {
        m = (frac | 0x0010000000000000ull) << 11;
        e = be - 1075 - 11;
    }
    pgx r;
    r.m = m;
    r.e = e + ex;
    return r;
}

// one bin as the host reads it, ldexpl((long double)lik, lik_exp): 0 at or below 2^-16446
PGX_FN pgx pgx_from_bin(double lik, int32_t lik_exp) {
    pgx r = pgx_from_double(lik, lik_exp);
    if (r.m == 0) return r;
    // x in [2^(e+63), 2^(e+64))
    if (r.e + 63 < PG_CALLS_ZERO_EXP || (r.e + 63 == PG_CALLS_ZERO_EXP && r.m == PGX_TOP)) return pgx_zero();
    return r;
}

// x < 2^p ?
PGX_FN bool pgx_below_pow2(pgx a, int32_t p) { return a.m == 0 || a.e + 64 <= p; }

// rounds the 128-bit fixed point hi.lo (hi normalised, bit 0 of lo may be a sticky bit) * 2^e to nearest even
PGX_FN pgx pgx_round(uint64_t hi, uint64_t lo, int32_t e) {
    const bool half = (lo >> 63) != 0;
    const bool rest = (lo << 1) != 0;
    if (half && (rest || (hi & 1ull))) {
        ++hi;
        if (hi == 0) { hi = PGX_TOP; ++e; }  // the carry out of rounding
    }
    pgx r;
    r.m = hi;
    r.e = e;
    return r;
}

// b.m moved right by d >= 0 bits inside a 128-bit window; what falls out of it is kept as `sticky`
PGX_FN void pgx_align(uint64_t bm, uint32_t d, uint64_t* hi, uint64_t* lo, bool* sticky) {
    *sticky = false;
    if (d == 0) { *hi = bm; *lo = 0; }
    else if (d < 64) { *hi = bm >> d; *lo = bm << (64 - d); }
    else if (d == 64) { *hi = 0; *lo = bm; }
    else if (d < 128) { *hi = 0; *lo = bm >> (d - 64); *sticky = (bm << (128 - d)) != 0; }
    else { *hi = 0; *lo = 0; *sticky = true; }
}

// a + b, rounded
PGX_FN pgx pgx_add(pgx a, pgx b) {
    if (a.m == 0) return b;
    if (b.m == 0) return a;
    if (a.e < b.e) { const pgx t = a; a = b; b = t; }
    const uint32_t d = (uint32_t)(a.e - b.e);
    uint64_t bh, bl;
    bool sticky;
    pgx_align(b.m, d, &bh, &bl, &sticky);
    uint64_t hi = a.m + bh;
    const bool carry = hi < bh;
    uint64_t lo = bl | (sticky ? 1ull : 0ull);
    int32_t e = a.e;
    if (carry) {
        lo = (lo >> 1) | (hi << 63) | (lo & 1ull);
        hi = (hi >> 1) | PGX_TOP;
        ++e;
    }
    return pgx_round(hi, lo, e);
}

// a - b for a >= b, rounded
PGX_FN pgx pgx_sub(pgx a, pgx b) {
    if (b.m == 0) return a;
    if (a.m == 0) return pgx_zero();
    const uint32_t d = (uint32_t)(a.e - b.e);
    uint64_t bh, bl;
    bool sticky;
    pgx_align(b.m, d, &bh, &bl, &sticky);
    // a.m.0 - bh.bl - (sticky: a little more, so one unit of the window less and a sticky bit back)
    uint64_t lo = 0ull - bl;
    uint64_t hi = a.m - bh - (bl != 0 ? 1ull : 0ull);
    if (sticky) {
        if (lo == 0) --hi;
        --lo;
    }
    if (hi == 0 && lo == 0) return pgx_zero();
    int32_t e = a.e;
    if (hi == 0) { hi = lo; lo = 0; e -= 64; }
    const int s = __builtin_clzll(hi);
    if (s) {
        hi = (hi << s) | (lo >> (64 - s));
        lo <<= s;
        e -= s;
    }
    if (sticky) lo |= 1ull;  // (only when d > 64: then s <= 1 and bit 0 is far below the rounding bit)
    return pgx_round(hi, lo, e);
}

PGX_FN pgx pgx_one_minus(pgx x) { return pgx_sub(pgx_one(), x); }

// a / b (b > 0), rounded: a 64-bit quotient of the mantissas by restoring division, the remainder decides the rounding
PGX_FN pgx pgx_div(pgx a, pgx b) {
    if (a.m == 0) return pgx_zero();
    uint64_t rem, nl;
    int32_t e;
    if (a.m >= b.m) { rem = a.m >> 1; nl = a.m << 63; e = a.e - b.e - 63; }   // quotient of (a.m 2^63) / b.m in [2^63, 2^64)
    else { rem = a.m; nl = 0; e = a.e - b.e - 64; }                          // ... of (a.m 2^64) / b.m
    uint64_t q = 0;
    for (int i = 0; i < 64; ++i) {
        const bool top = (rem >> 63) != 0;
        rem = (rem << 1) | (nl >> 63);
        nl <<= 1;
        q <<= 1;
        if (top || rem >= b.m) { rem -= b.m; q |= 1ull; }
    }
    // rem < b.m: 2 rem against b.m without overflow
    const uint64_t other = b.m - rem;
    if (rem > other || (rem == other && (q & 1ull))) {
        ++q;
        if (q == 0) { q = PGX_TOP; ++e; }
    }
    pgx r;
    r.m = q;
    r.e = e;
    return r;
}

// The reference's tie threshold: the `double` literal 0.0000000001 widened (src/genotypingresult.cpp:171)
PGX_FN pgx pgx_tie_threshold() { return pgx_from_double(0.0000000001, 0); }

// Genotype quality of prob_wrong = 1 - best from the threshold table (thr_m / thr_e [PG_GQ_STEPS], descending:
// entry k = the largest long double x with (size_t)(-10 log10l(x)) >= k): the largest k with prob_wrong <= entry k.
PGX_FN uint32_t pgx_gq(pgx prob_wrong, const uint64_t* thr_m, const int32_t* thr_e) {
    if (prob_wrong.m == 0) return PG_GQ_CERTAIN;
    uint32_t lo = 0, hi = PG_GQ_STEPS - 1;   // prob_wrong <= 1 = entry 0
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        pgx t;
        t.m = thr_m[mid];
        t.e = thr_e[mid];
        if (pgx_cmp(prob_wrong, t) <= 0) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------------------------
//  One variant's call from its bins: the rules of DESIGN.md 4e.  `Keys` walks the keys of the reference's map in the
//  map's order — start(), then next(&value) until it answers false, value as pgx_from_bin gives it — and is walked
//  three times instead of keeping the values (an array indexed at run time would live in scratch memory).
// ---------------------------------------------------------------------------------------------------------------
#define PGX_CALL_OK 0u
#define PGX_CALL_NONE 1u
#define PGX_CALL_NOT_UNIQUE 2u
#define PGX_CALL_DEFERRED 3u

struct pgx_decision {
    uint32_t flags;   // PGX_CALL_*
    uint32_t best;    // number of the likeliest genotype's key in walking order (PGX_CALL_OK only)
    uint32_t gq;
};

PGX_FN uint32_t pgx_gq_of_best(pgx best, const uint64_t* thr_m, const int32_t* thr_e) {
    const pgx one = pgx_one();
    if (pgx_cmp(best, one) >= 0) return PG_GQ_CERTAIN;
    return pgx_gq(pgx_sub(one, best), thr_m, thr_e);
}

// |a - b| < the tie threshold
PGX_FN bool pgx_within_tie(pgx a, pgx b) {
    const pgx d = pgx_cmp(a, b) >= 0 ? pgx_sub(a, b) : pgx_sub(b, a);
    return pgx_cmp(d, pgx_tie_threshold()) < 0;
}

template <class Keys>
PGX_FN pgx_decision pgx_decide(Keys& keys, const uint64_t* thr_m, const int32_t* thr_e) {
    pgx_decision r;
    r.flags = PGX_CALL_NONE;
    r.best = 0;
    r.gq = 0;
    pgx v, sum = pgx_zero(), largest = pgx_zero();
    keys.start();
    while (keys.next(&v)) {   // GenotypingResult::normalize: the keys added one after the other
        sum = pgx_add(sum, v);
        if (pgx_cmp(v, largest) > 0) largest = v;
    }
    if (sum.m == 0) return r;   // no key, or every bin zero: best == 0
    if (pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) { r.flags = PGX_CALL_DEFERRED; return r; }
    pgx best = pgx_zero();
    uint32_t i = 0;
    keys.start();
    while (keys.next(&v)) {   // get_likeliest_genotype: `>=`, the last of equal maxima (which the tie rule then refuses)
        const pgx q = pgx_div(v, sum);
        if (pgx_cmp(q, best) >= 0) { best = q; r.best = i; }
        ++i;
    }
    i = 0;
    keys.start();
    while (keys.next(&v)) {
        if (i != r.best && pgx_within_tie(best, pgx_div(v, sum))) { r.flags = PGX_CALL_NOT_UNIQUE; return r; }
        ++i;
    }
    r.flags = PGX_CALL_OK;
    r.gq = pgx_gq_of_best(best, thr_m, thr_e);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
//  One VCF record's call from its bubble's bins: the rules of DESIGN.md 4e "Records".  A bubble that the index builder
//  merged from several records is taken apart again as Graph::write_genotypes does it: the bubble's normalised values
//  are folded onto the record's own alleles (Variant::separate_variants), genotypes over alleles of undefined sequence
//  are dropped and the rest renormalised (get_specific_likelihoods), then likeliest genotype and quality as above.
//
//  `Keys` walks the bubble's keys in the map's order — start(), then next(&value, &key) until it answers false — with
//  key = (ra << 16) | rb, ra <= rb the record alleles the key's two bubble alleles carry.  The folded map F is never
//  kept: its keys are visited in ascending order, and each visit walks the bubble once, adding the quotients that fall
//  onto that key in the bubble's order (one division per bubble key and walk) and noting the next key on the way.
//  `defined(ra)`: the record allele has a defined sequence (asked only if has_undefined).
// ---------------------------------------------------------------------------------------------------------------
#define PGX_CALL_EMPTY 0x100u   // with PGX_CALL_OK: 0/0, GQ 10000 from a bubble without keys (F[(0,0)] = 1), not from evidence
#define PGX_NO_KEY 0xFFFFFFFFFFFFFFFFull

struct pgx_record_decision {
    uint32_t flags;   // PGX_CALL_* (| PGX_CALL_EMPTY)
    uint32_t key;     // (ra << 16) | rb of the likeliest genotype (PGX_CALL_OK only)
    uint32_t gq;
};

// F[cur] (if `value`) and the smallest key above cur; cur == PGX_NO_KEY: only the smallest key of all
template <class Keys>
PGX_FN pgx pgx_fold_key(Keys& keys, pgx sum, uint64_t cur, bool value, uint64_t* next) {
    pgx acc = pgx_zero(), v;
    uint32_t k;
    uint64_t nxt = PGX_NO_KEY;
    keys.start();
    while (keys.next(&v, &k)) {
        if (k == cur) { if (value) acc = pgx_add(acc, pgx_div(v, sum)); }
        else if ((cur == PGX_NO_KEY || k > cur) && k < nxt) nxt = k;
    }
    *next = nxt;
    return acc;
}

// Best and runner-up of a sequence taken with `>=`: `best` is the LAST of equal maxima, `second` the largest other value
// (equal to best for equal maxima).  |x - best| < t holds for some other x iff it holds for `second`: rounded subtraction
// is monotone.
struct pgx_top2 {
    pgx best, second;
    uint64_t best_key;
    bool has_second;
};
PGX_FN void pgx_top2_init(pgx_top2* t) { t->best = pgx_zero(); t->second = pgx_zero(); t->best_key = PGX_NO_KEY; t->has_second = false; }
PGX_FN void pgx_top2_take(pgx_top2* t, pgx x, uint64_t key) {
    if (pgx_cmp(x, t->best) >= 0) {
        if (t->best_key != PGX_NO_KEY) { t->second = t->best; t->has_second = true; }
        t->best = x;
        t->best_key = key;
    } else {
        if (!t->has_second || pgx_cmp(x, t->second) > 0) t->second = x;
        t->has_second = true;
    }
}

template <class Keys, class Defined>
PGX_FN pgx_record_decision pgx_decide_record(Keys& keys, bool has_undefined, Defined& defined, const uint64_t* thr_m, const int32_t* thr_e) {
    pgx_record_decision r;
    r.flags = PGX_CALL_NONE;
    r.key = 0;
    r.gq = 0;
    pgx v, sum = pgx_zero(), largest = pgx_zero();
    uint32_t k, n = 0;
    keys.start();
    while (keys.next(&v, &k)) {   // GenotypingResult::normalize of the bubble
        sum = pgx_add(sum, v);
        if (pgx_cmp(v, largest) > 0) largest = v;
        ++n;
    }
    if (n == 0) {   // an empty map: F[(0,0)] = 1 (allele 0 is always defined: 1 / 1 after get_specific_likelihoods)
        r.flags = PGX_CALL_OK | PGX_CALL_EMPTY;
        r.gq = PG_GQ_CERTAIN;
        return r;
    }
    if (sum.m == 0) return r;   // every bin zero: nothing is normalised, best == 0
    if (pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) { r.flags = PGX_CALL_DEFERRED; return r; }
    uint64_t first, cur, next;
    (void)pgx_fold_key(keys, sum, PGX_NO_KEY, false, &first);
    pgx sum2 = pgx_zero();
    if (has_undefined) {   // get_specific_likelihoods: the defined keys of F added in F's order
        for (cur = first; cur != PGX_NO_KEY; cur = next) {
            const bool def = defined((uint32_t)(cur >> 16)) && defined((uint32_t)(cur & 0xFFFFu));
            const pgx f = pgx_fold_key(keys, sum, cur, def, &next);
            if (def) sum2 = pgx_add(sum2, f);
        }
        if (sum2.m == 0) return r;   // no defined key, or all of them zero: best == 0
    }
    pgx_top2 t;
    pgx_top2_init(&t);
    for (cur = first; cur != PGX_NO_KEY; cur = next) {   // get_likeliest_genotype over F
        const bool def = !has_undefined || (defined((uint32_t)(cur >> 16)) && defined((uint32_t)(cur & 0xFFFFu)));
        pgx f = pgx_fold_key(keys, sum, cur, def, &next);
        if (!def) continue;
        if (has_undefined) f = pgx_div(f, sum2);
        pgx_top2_take(&t, f, cur);
    }
    if (t.best.m == 0) return r;
    if (t.has_second && pgx_within_tie(t.best, t.second)) { r.flags = PGX_CALL_NOT_UNIQUE; return r; }
    r.flags = PGX_CALL_OK;
    r.key = (uint32_t)t.best_key;
    r.gq = pgx_gq_of_best(t.best, thr_m, thr_e);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
//  Genotype likelihoods as the VCF prints them (the GL column): four significant decimal digits of
//  log10l(L), which is what `ostream << setprecision(4)` shows of it.  The likelihood L itself is formed in the integer
//  pairs above, bit for bit the host's long double; only the logarithm and its digits are fp64.
//
//  The route and its error, in units of u = 2^-53 relative to y = |log10 x| (x = m 2^e, E = e + 64):
//    E == 0   x = 1 - d 2^-64, d = 2^64 - m an exact integer: (double)d 1u, log1p L ulp = 2L u, the division by the rounded
//             ln 10 1.5u;                                                                                    2.5u + 2L u
//    E == 1   x = 1 + d 2^-63, the same with the sign of the logarithm positive;                             2.5u + 2L u
//    E <  0   y = -(E c_hi + (E c_lo + log10(m 2^-64))): E c_hi is exact (15 x 37 bits), both terms are <= 0 so nothing
//             cancels and every absolute error is relative to y or less: (double)m 1u / ln 10 of the argument = 0.44u
//             absolute, against y >= log10 2: 1.5u; log10 L ulp = 2L u; E c_lo and the two additions 3u;    4.5u + 2L u
//    digits   s = (y 10^n1) 10^n2 with n1, n2 <= 12, both powers exact doubles: two products, 2u.
//  With L = 4 ulp for log10 and log1p (the device compiler's documentation promises fewer: the bound is taken with room)
//  the relative error of s is below 14.5u < 16u = 1.78e-15, and s < 10^4: |s - exact| < 1.78e-11.  A digit is decided here
//  only if s is further than PG_GL_WINDOW = 1e-9 from a rounding boundary .5 — 56 times the bound (at least 16 are asked
//  for) — and is left to the host otherwise (PG_GL_DEFERRED): exact ties included, and about 2e-9 of all values.
// ---------------------------------------------------------------------------------------------------------------
#include <math.h>

#ifndef PG_GL_DEFINED   // (the same in include/pangenie_hmm.h)
#define PG_GL_DEFINED
typedef struct pg_gl { int16_t mant; int16_t exp10; } pg_gl;
#define PG_GL_NEG_INF  (-32768)
#define PG_GL_DEFERRED (-32767)
#endif

#define PG_GL_WINDOW 1e-9
#define PGX_LOG10_2_HI 0x1.34413509fp-2          // the first 37 bits of log10 2
#define PGX_LOG10_2_LO 0x1.e7fbcc47c4acdp-40     // log10 2 - PGX_LOG10_2_HI
#define PGX_LN_10 0x1.26bb1bbb55516p+1

PGX_FN pg_gl pgx_gl_of(int mant, int exp10) { pg_gl g; g.mant = (int16_t)mant; g.exp10 = (int16_t)exp10; return g; }
PGX_FN pg_gl pgx_gl_neg_inf() { return pgx_gl_of(0, PG_GL_NEG_INF); }
PGX_FN pg_gl pgx_gl_deferred() { return pgx_gl_of(0, PG_GL_DEFERRED); }
PGX_FN bool pgx_gl_is_deferred(pg_gl g) { return g.mant == 0 && g.exp10 == PG_GL_DEFERRED; }

// y * 10^n, 0 <= n <= 24: two products with exact powers of ten
PGX_FN double pgx_gl_scale(double y, int n) {
    const int n1 = n < 12 ? n : 12, n2 = n - n1;
    double p1 = 1.0, p2 = 1.0;
    for (int i = 0; i < n1; ++i) p1 *= 10.0;
    for (int i = 0; i < n2; ++i) p2 *= 10.0;
    return (y * p1) * p2;
}

// the four digits of log10(x); a nonzero x below 2^PG_CALLS_DEFER_EXP (the host's quotient there would be subnormal or 0)
// and a value within PG_GL_WINDOW of a rounding boundary are PG_GL_DEFERRED
PGX_FN pg_gl pgx_gl(pgx x) {
    if (x.m == 0) return pgx_gl_neg_inf();
    if (pgx_below_pow2(x, PG_CALLS_DEFER_EXP)) return pgx_gl_deferred();
    const int32_t E = x.e + 64;
    if (E == 1 && x.m == PGX_TOP) return pgx_gl_of(0, 0);
    double y;
    bool positive = false;
    if (E == 0) y = -log1p(-((double)(0ull - x.m) * 0x1p-64)) / PGX_LN_10;
    else if (E == 1) { y = log1p((double)(x.m - PGX_TOP) * 0x1p-63) / PGX_LN_10; positive = true; }
    else if (E < 0) y = -((double)E * PGX_LOG10_2_HI + ((double)E * PGX_LOG10_2_LO + log10((double)x.m * 0x1p-64)));
    else return pgx_gl_deferred();   // x >= 2: no likelihood
    int k = (int)floor(log10(y));
    double s = 0.0;
    for (int it = 0; it < 3; ++it) {   // k until s lies in [1000, 10000)
        if (k > 3 || k < -21) return pgx_gl_deferred();   // (y in [2.3e-20, 4951]: not reached)
        s = pgx_gl_scale(y, 3 - k);
        if (s < 1000.0) --k;
        else if (s >= 10000.0) ++k;
        else break;
    }
    if (!(s >= 1000.0 && s < 10000.0)) return pgx_gl_deferred();
    const double fl = floor(s), fr = s - fl;
    if (fabs(fr - 0.5) < PG_GL_WINDOW) return pgx_gl_deferred();
    int r = (int)fl + (fr > 0.5 ? 1 : 0);
    if (r == 10000) { r = 1000; ++k; }
    return pgx_gl_of(positive ? r : -r, k);
}

// ---------------------------------------------------------------------------------------------------------------
//  One VCF record's GL values from its bubble's bins.  The likelihoods are those of pgx_decide_record: the bubble's sum,
//  one pgx_div per key, the additions onto one record key in the bubble's order, and for a record with undefined alleles
//  sum2 over the defined keys in (ra, rb) order and a second pgx_div if sum2 > 0.  The record's defined genotype pairs are
//  enumerated in (ra, rb) order, each one walk of the bubble's keys (a key nothing folds onto adds 0 to sum2, which changes
//  no rounding, and reads -inf).  `vcf(a)`: index of record allele a among the defined ones, 0xFFFF if undefined;
//  `out(i, g)`: value i of the record, genotype (a <= b) over defined-allele indices at b (b + 1) / 2 + a.
// ---------------------------------------------------------------------------------------------------------------
template <class Keys, class Vcf, class Out>
PGX_FN void pgx_record_gl(Keys& keys, uint32_t n_alleles, bool has_undefined, Vcf& vcf, Out& out) {
    pgx v, sum = pgx_zero(), largest = pgx_zero();
    uint32_t k, n = 0, nd = 0;
    for (uint32_t a = 0; a < n_alleles; ++a) nd += vcf(a) != 0xFFFFu ? 1u : 0u;
    const uint32_t n_values = nd * (nd + 1u) / 2u;
    keys.start();
    while (keys.next(&v, &k)) {   // GenotypingResult::normalize of the bubble
        sum = pgx_add(sum, v);
        if (pgx_cmp(v, largest) > 0) largest = v;
        ++n;
    }
    if (n == 0 || sum.m == 0 || pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) {
        // an empty map: F[(0,0)] = 1; every bin zero: nothing is normalised, every value 0; below the cut: the host's
        const pg_gl g = (n == 0 || sum.m == 0) ? pgx_gl_neg_inf() : pgx_gl_deferred();
        for (uint32_t i = 0; i < n_values; ++i) out(i, (n == 0 && i == 0) ? pgx_gl_of(0, 0) : g);
        return;
    }
    uint64_t next;
    pgx sum2 = pgx_zero();
    if (has_undefined)   // get_specific_likelihoods: the defined keys of F added in F's order
        for (uint32_t ra = 0; ra < n_alleles; ++ra) {
            if (vcf(ra) == 0xFFFFu) continue;
            for (uint32_t rb = ra; rb < n_alleles; ++rb)
                if (vcf(rb) != 0xFFFFu) sum2 = pgx_add(sum2, pgx_fold_key(keys, sum, ((uint64_t)ra << 16) | rb, true, &next));
        }
    for (uint32_t ra = 0; ra < n_alleles; ++ra) {
        const uint32_t va = vcf(ra);
        if (va == 0xFFFFu) continue;
        for (uint32_t rb = ra; rb < n_alleles; ++rb) {
            const uint32_t vb = vcf(rb);
            if (vb == 0xFFFFu) continue;
            pgx f = pgx_fold_key(keys, sum, ((uint64_t)ra << 16) | rb, true, &next);
            if (sum2.m != 0) f = pgx_div(f, sum2);
            out(vb * (vb + 1u) / 2u + va, pgx_gl(f));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
//  The text of one VCF record's sample column, `GT:GQ:GL:KC`: what Graph::genotypes_records prints of a
//  record's call, its GL values and its bubble's coverage.  Pure integer formatting, one rule for the kernels of
//  pg_record_text.hip and for the host.  The text has no terminator and no separator; it is, in order,
//    1. `a1/a2:gq:` if (flags & 0xFF) == PGX_CALL_OK and not no_call (PGX_CALL_EMPTY prints like OK: 0/0:10000:), else `.:.:`
//    2. the n_gl values as pgx_gl_text prints them, joined by `,`
//    3. `:` and kc in decimal.
//  A record is THE HOST'S — length 0, nothing written — if its call is PGX_CALL_DEFERRED, if one of its values is
//  PG_GL_DEFERRED or one pgx_gl_text refuses, or if n_gl < 3 (the host throws "too few likelihoods" for it).
//  Every character goes through a sink's put(): one that counts gives the length, one that stores gives the text, so the
//  two cannot differ; no array is indexed at run time (on the device it would be scratch memory).
// ---------------------------------------------------------------------------------------------------------------
#ifndef PG_CALL_DEFINED   // (the same in include/pangenie_hmm.h)
#define PG_CALL_DEFINED
typedef struct pg_call { uint16_t allele_1, allele_2; uint16_t gq; uint16_t flags; } pg_call;
#endif

#if defined(__HIP__)
#define PGX_MEM __host__ __device__
#else
#define PGX_MEM
#endif

struct pgx_count_sink {
    uint32_t n;
    PGX_MEM void put(char) { ++n; }
};
struct pgx_buf_sink {
    char* p;
    uint32_t n;
    PGX_MEM void put(char c) { p[n++] = c; }
};

// 255/255:10000: is 14 bytes, a value at most 10 (-1.234e-05, -0.0001234), n_gl - 1 commas, :65535 is 6
#define PGX_TEXT_PER_RECORD 19u
#define PGX_TEXT_PER_VALUE 11u
PGX_FN uint64_t pgx_record_text_bound(uint64_t n_records, uint64_t n_gl_total) { return PGX_TEXT_PER_RECORD * n_records + PGX_TEXT_PER_VALUE * n_gl_total; }

template <class Sink>
PGX_FN void pgx_put_uint(uint32_t v, Sink& s) {
    uint32_t div = 1;
    while (v / div >= 10u) div *= 10u;
    for (; div; div /= 10u) s.put((char)('0' + (v / div) % 10u));
}

// a value pgx_gl_text answers -1 for
PGX_FN bool pgx_gl_refused(pg_gl g) {
    if (g.mant == 0) return !(g.exp10 == PG_GL_NEG_INF || g.exp10 == 0);
    const int a = g.mant < 0 ? -(int)g.mant : (int)g.mant;
    return a < 1000 || a > 9999 || g.exp10 < -99 || g.exp10 > 99;
}

// the characters of pgx_gl_text, for a value that is not refused
template <class Sink>
PGX_FN void pgx_gl_put(pg_gl g, Sink& s) {
    if (g.mant == 0) {
        if (g.exp10 == 0) s.put('0');
        else { s.put('-'); s.put('i'); s.put('n'); s.put('f'); }
        return;
    }
    const int a = g.mant < 0 ? -(int)g.mant : (int)g.mant;
    const int X = g.exp10;
    const int d0 = a / 1000, d1 = (a / 100) % 10, d2 = (a / 10) % 10, d3 = a % 10;
    const int nd = d3 ? 4 : d2 ? 3 : d1 ? 2 : 1;   // trailing zeros stripped
#define PGX_DIGIT(i) ((char)('0' + ((i) == 0 ? d0 : (i) == 1 ? d1 : (i) == 2 ? d2 : d3)))
    if (g.mant < 0) s.put('-');
    if (X < -4 || X >= 4) {
        s.put(PGX_DIGIT(0));
        if (nd > 1) { s.put('.'); for (int i = 1; i < nd; ++i) s.put(PGX_DIGIT(i)); }
        s.put('e');
        s.put(X < 0 ? '-' : '+');
        const int ax = X < 0 ? -X : X;
        s.put((char)('0' + ax / 10));
        s.put((char)('0' + ax % 10));
    } else if (X >= 0) {
        for (int i = 0; i <= X; ++i) s.put(i < nd ? PGX_DIGIT(i) : '0');
        if (nd > X + 1) { s.put('.'); for (int i = X + 1; i < nd; ++i) s.put(PGX_DIGIT(i)); }
    } else {
        s.put('0'); s.put('.');
        for (int i = 0; i < -X - 1; ++i) s.put('0');
        for (int i = 0; i < nd; ++i) s.put(PGX_DIGIT(i));
    }
#undef PGX_DIGIT
}

// is the record the host's?  (the values are looked at only if the call and n_gl do not already say so)
PGX_FN bool pgx_record_is_hosts(pg_call call, const pg_gl* gl, uint32_t n_gl) {
    if ((call.flags & 0xFFu) == PGX_CALL_DEFERRED || n_gl < 3u) return true;
    for (uint32_t i = 0; i < n_gl; ++i)
        if (pgx_gl_refused(gl[i])) return true;
    return false;
}

// the three parts of a record that is not the host's
template <class Sink>
PGX_FN void pgx_record_head_put(pg_call call, bool no_call, Sink& s) {
    if ((call.flags & 0xFFu) == PGX_CALL_OK && !no_call) {
        pgx_put_uint(call.allele_1, s); s.put('/'); pgx_put_uint(call.allele_2, s); s.put(':'); pgx_put_uint(call.gq, s); s.put(':');
    } else { s.put('.'); s.put(':'); s.put('.'); s.put(':'); }
}
template <class Sink>
PGX_FN void pgx_record_tail_put(uint32_t kc, Sink& s) { s.put(':'); pgx_put_uint(kc, s); }
template <class Sink>
PGX_FN void pgx_record_put(pg_call call, const pg_gl* gl, uint32_t n_gl, uint32_t kc, bool no_call, Sink& s) {
    pgx_record_head_put(call, no_call, s);
    for (uint32_t i = 0; i < n_gl; ++i) {
        if (i) s.put(',');
        pgx_gl_put(gl[i], s);
    }
    pgx_record_tail_put(kc, s);
}

// the length of the record's text; 0: the host's
PGX_FN uint32_t pgx_record_text_len(pg_call call, const pg_gl* gl, uint32_t n_gl, uint32_t kc, bool no_call) {
    if (pgx_record_is_hosts(call, gl, n_gl)) return 0;
    pgx_count_sink s;
    s.n = 0;
    pgx_record_put(call, gl, n_gl, kc, no_call, s);
    return s.n;
}
// writes the text to buf (pgx_record_text_bound(1, n_gl) bytes suffice for GT numbers up to 255 and a GQ up to 10000);
// the length, 0 and nothing written for the host's
PGX_FN uint32_t pgx_record_text(pg_call call, const pg_gl* gl, uint32_t n_gl, uint32_t kc, bool no_call, char* buf) {
    if (pgx_record_is_hosts(call, gl, n_gl)) return 0;
    pgx_buf_sink s;
    s.p = buf;
    s.n = 0;
    pgx_record_put(call, gl, n_gl, kc, no_call, s);
    return s.n;
}

// ---------------------------------------------------------------------------------------------------------------
//  Host only: the pair <-> long double, and the threshold table from log10l itself.
// ---------------------------------------------------------------------------------------------------------------
#include <math.h>
#include <stddef.h>

static inline long double pgx_to_ld(pgx a) { return ldexpl((long double)a.m, a.e); }
static inline pgx pgx_from_ld(long double x) {   // exact for a normal or zero x >= 0
    if (!(x > 0.0L)) return pgx_zero();
    int ex = 0;
    const long double f = frexpl(x, &ex);        // f in [0.5, 1)
    pgx r;
    r.m = (uint64_t)ldexpl(f, 64);
    r.e = ex - 64;
    return r;
}
static inline size_t pgx_gq_host(long double prob_wrong) { return (size_t)(-10.0L * log10l(prob_wrong)); }

// entry k = the largest long double x <= 1 with (size_t)(-10 log10l(x)) >= k, found with nextafterl from 10^(-k/10).
// Returns 0, or -1 if the search did not end (log10l not monotone there: the table would not be the host's truncation).
static inline int pgx_build_gq_table(uint64_t* thr_m, int32_t* thr_e) {
    for (int k = 0; k < PG_GQ_STEPS; ++k) {
        long double x = 1.0L;
        if (k > 0) {
            x = powl(10.0L, -(long double)k / 10.0L);
            int guard = 0;
            while (pgx_gq_host(x) < (size_t)k) { x = nextafterl(x, 0.0L); if (++guard > 100000) return -1; }
            for (;;) {
                const long double up = nextafterl(x, 2.0L);
                if (!(up < 1.0L) || pgx_gq_host(up) < (size_t)k) break;
                x = up;
                if (++guard > 100000) return -1;
            }
        }
        const pgx t = pgx_from_ld(x);
        thr_m[k] = t.m;
        thr_e[k] = t.e;
    }
    return 0;
}

// The text of a GL value: what `ostream << setprecision(4)` prints of the long double logarithm, i.e. "%.4g" of the decimal
// mant 10^(exp10 - 3) — "-inf", "0", fixed notation with trailing zeros stripped for exp10 in [-4, 3], else d.ddde-XX.
// Returns the length, or -1 for PG_GL_DEFERRED, a value that is none, or a buffer too small (32 bytes always suffice).
static inline int pgx_gl_text(pg_gl g, char* buf, size_t len) {
    char t[32];
    int n = 0;
    if (g.mant == 0) {
        if (g.exp10 == PG_GL_NEG_INF) { t[0] = '-'; t[1] = 'i'; t[2] = 'n'; t[3] = 'f'; n = 4; }
        else if (g.exp10 == 0) t[n++] = '0';
        else return -1;
    } else {
        int a = g.mant < 0 ? -(int)g.mant : (int)g.mant;
        const int X = g.exp10;
        if (a < 1000 || a > 9999 || X < -99 || X > 99) return -1;
        char d[4];
        for (int i = 3; i >= 0; --i) { d[i] = (char)('0' + a % 10); a /= 10; }
        int nd = 4;
        while (nd > 1 && d[nd - 1] == '0') --nd;
        if (g.mant < 0) t[n++] = '-';
        if (X < -4 || X >= 4) {
            t[n++] = d[0];
            if (nd > 1) { t[n++] = '.'; for (int i = 1; i < nd; ++i) t[n++] = d[i]; }
            t[n++] = 'e';
            t[n++] = X < 0 ? '-' : '+';
            const int ax = X < 0 ? -X : X;
            t[n++] = (char)('0' + ax / 10);
            t[n++] = (char)('0' + ax % 10);
        } else if (X >= 0) {
            for (int i = 0; i <= X; ++i) t[n++] = i < nd ? d[i] : '0';
            if (nd > X + 1) { t[n++] = '.'; for (int i = X + 1; i < nd; ++i) t[n++] = d[i]; }
        } else {
            t[n++] = '0'; t[n++] = '.';
            for (int i = 0; i < -X - 1; ++i) t[n++] = '0';
            for (int i = 0; i < nd; ++i) t[n++] = d[i];
        }
    }
    if (!buf || (size_t)n + 1 > len) return -1;
    for (int i = 0; i < n; ++i) buf[i] = t[i];
    buf[n] = 0;
    return n;
}
