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
