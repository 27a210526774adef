// pg_combine.h — the arithmetic of the path-subset flow on the device: pg_combine.hip, DESIGN.md §4e-4.
//
// The reference's `-a` option genotypes a chromosome once per subset of paths and adds the subsets' UNNORMALISED
// likelihoods per genotype key (run_genotyping, src/commands.cpp:163-177; GenotypingResult::combine,
// src/genotypingresult.cpp:193-198: map[key] += value) before it normalises once.  Here the chains of one group are
// folded key by key in the integer pairs of pg_calls.h, in the order the caller lists the chains in:
//     ((0 + L_s1) + L_s2) + L_s3 ...  over the chains that HOLD the key, every addition rounded to 64 bits, ties to even
// (0.0L + x = x is exact).  The set of keys is the union over the chains: presence belongs to the combined bin.
//
// Summands.  pgx_from_bin keeps the 53 bits of a bin whatever its exponent; the host's ldexpl((long double)lik, lik_exp)
// rounds a value below 2^-16382 to a multiple of the smallest subnormal, 2^-16445 (ties to even).  pgc_summand repeats
// that rounding, so a summand here IS the host's long double, subnormal ones included.  pgx_add then needs nothing
// more: every long double is a multiple of 2^-16445, so is every exact partial sum, and the x87 rounds such a sum only
// when it needs more than 64 bits — then it is a normal number and the rounding is pgx_round's; below that both are exact.
//
// Deferral.  A key is PG_COMBINED_DEFERRED iff its largest nonzero summand lies below 2^PG_CALLS_DEFER_EXP, the cut of
// the calls.  The argument one might give for the cut alone — "a summand of the subnormal range lies at least 82 bits
// below a summand at or above 2^-16300, so it reaches an addition only as a sticky bit, never as the half bit" — does
// NOT hold once a third summand lies between the two.  (mid + tiny) + large with large = 2^-16300, mid = 2^-16364 (the
// half bit of large) and tiny = 2^-16428 (1 + 2^-20): the host reads tiny as 2^-16428, half an ulp of mid, so mid + tiny
// is a tie and stays mid, and large + mid is a tie and stays large; with all 53 bits of tiny both ties round up.  It is
// the exact summand above, not the cut, that makes every key that is not flagged equal the x87's sum; the cut keeps the
// calls away from quotients next to the subnormals, as in pg_calls.h.  tests/cpp/test_combine_arith.cpp checks the
// rule, the example and a million random keys against the x87.
#pragma once
#include "pg_calls.h"

#ifndef PG_COMBINED_DEFINED   // (the same in include/pangenie_hmm.h)
#define PG_COMBINED_DEFINED
typedef struct pg_combined_bin { uint64_t m; int32_t e; uint32_t flags; } pg_combined_bin;
#define PG_COMBINED_PRESENT  1u
#define PG_COMBINED_DEFERRED 2u
#endif

#define PGC_LD_QUANTUM_EXP (-16445)   // the smallest subnormal long double is 2^-16445

#if defined(__HIP__)
#define PGC_MEMBER __host__ __device__
#else
#define PGC_MEMBER
#endif

// one bin as the host reads it, ldexpl((long double)lik, lik_exp), subnormal results rounded as ldexpl rounds them
PGX_FN pgx pgc_summand(double lik, int32_t lik_exp) {
    pgx r = pgx_from_double(lik, lik_exp);
    if (r.m == 0 || r.e >= PGC_LD_QUANTUM_EXP) return r;
    const uint32_t d = (uint32_t)(PGC_LD_QUANTUM_EXP - r.e);   // bits of r.m below the quantum
    if (d > 64) return pgx_zero();                             // below half the quantum
    uint64_t q, rem;
    if (d == 64) { q = 0; rem = r.m; }
    else { q = r.m >> d; rem = r.m << (64 - d); }
    if ((rem >> 63) && ((rem << 1) != 0 || (q & 1ull))) ++q;
    if (q == 0) return pgx_zero();
    const int s = __builtin_clzll(q);
    r.m = q << s;
    r.e = PGC_LD_QUANTUM_EXP - s;
    return r;
}

// One key's fold over the chains of a group, in their order.
struct pgc_fold {
    pgx sum, largest;
    uint32_t held;   // a chain holds the key
};
PGX_FN void pgc_fold_init(pgc_fold* f) { f->sum = pgx_zero(); f->largest = pgx_zero(); f->held = 0; }
PGX_FN void pgc_fold_take(pgc_fold* f, pgx x) {
    f->sum = pgx_add(f->sum, x);
    if (pgx_cmp(x, f->largest) > 0) f->largest = x;
    f->held = 1;
}
PGX_FN pg_combined_bin pgc_fold_bin(const pgc_fold* f) {
    pg_combined_bin b;
    b.m = 0; b.e = 0; b.flags = 0;
    if (!f->held) return b;
    b.flags = PG_COMBINED_PRESENT;
    if (f->largest.m != 0 && pgx_below_pow2(f->largest, PG_CALLS_DEFER_EXP)) { b.flags |= PG_COMBINED_DEFERRED; return b; }
    if (f->sum.m != 0) { b.m = f->sum.m; b.e = f->sum.e; }
    return b;
}

// The keys of one variant's combined map for pgx_decide: its present bins in bin order (allele slots a <= b, row after
// row).  A PG_COMBINED_DEFERRED bin reads 0 and sets `deferred`: the caller answers PGX_CALL_DEFERRED whatever pgx_decide says.
struct pgc_keys {
    const pg_combined_bin* bins;   // the variant's first bin
    uint32_t n;                    // A (A + 1) / 2
    uint32_t i;
    bool deferred;
    PGC_MEMBER void start() { i = 0; }
    PGC_MEMBER bool next(pgx* v) {
        while (i < n) {
            const pg_combined_bin b = bins[i++];
            if (!(b.flags & PG_COMBINED_PRESENT)) continue;
            if (b.flags & PG_COMBINED_DEFERRED) { deferred = true; *v = pgx_zero(); return true; }
            v->m = b.m;
            v->e = b.m ? b.e : 0;
            return true;
        }
        return false;
    }
    // the bin of key number k (walking order)
    PGC_MEMBER uint32_t bin_of(uint32_t k) const {
        uint32_t seen = 0, at = 0;
        for (uint32_t j = 0; j < n; ++j)
            if (bins[j].flags & PG_COMBINED_PRESENT) {
                if (seen == k) at = j;
                ++seen;
            }
        return at;
    }
};

// The keys of one variant's combined map for pgx_decide_record and pgx_record_gl: the present bins in bin
// order as pgc_keys walks them, each with the record alleles its two slots carry — key = (ra << 16) | rb, ra <= rb.
// Presence is the bin's flag: the union over the chains knows no allele mask (subsets that carry {0,1} and {0,2} leave no
// key (1,2)).  A PG_COMBINED_DEFERRED bin reads 0; the caller asks any_deferred() first and answers for the whole variant.
// `Own`: own(s) = the record allele of slot s.  The lane-per-record kernels keep a byte per slot in one 64-bit register
// (pgc_own_packed: at most 8 slots, PG_AMAX is 5); tests/cpp/test_combined_records_arith.cpp walks wider bubbles over an array.
struct pgc_own_packed {
    unsigned long long w;   // byte s: the record allele of slot s
    PGC_MEMBER uint32_t operator()(uint32_t s) const { return (uint32_t)(w >> (8u * s)) & 0xFFu; }
};
struct pgc_own_array {
    const uint16_t* of_slot;
    PGC_MEMBER uint32_t operator()(uint32_t s) const { return of_slot[s]; }
};
template <class Own>
struct pgc_record_keys_of {
    const pg_combined_bin* bins;   // the variant's first bin
    uint32_t A;
    Own own;
    uint32_t a, b, bin;
    PGC_MEMBER void start() { a = 0; b = 0; bin = 0; }
    PGC_MEMBER bool next(pgx* v, uint32_t* key) {
        while (a < A) {
            const uint32_t ca = a, cb = b;
            const pg_combined_bin x = bins[bin++];
            if (++b == A) { ++a; b = a; }
            if (!(x.flags & PG_COMBINED_PRESENT)) continue;
            const uint32_t oa = own(ca), ob = own(cb);
            const bool value = !(x.flags & PG_COMBINED_DEFERRED) && x.m != 0;
            v->m = value ? x.m : 0;
            v->e = value ? x.e : 0;
            *key = oa <= ob ? (oa << 16) | ob : (ob << 16) | oa;
            return true;
        }
        return false;
    }
    PGC_MEMBER bool any_deferred() const {
        bool d = false;
        for (uint32_t i = 0; i < A * (A + 1u) / 2u; ++i) d = d || (bins[i].flags & PG_COMBINED_DEFERRED) != 0;
        return d;
    }
};
typedef pgc_record_keys_of<pgc_own_packed> pgc_record_keys;

// allele slots (a <= b) of bin number `bin` of a variant with A alleles
PGX_FN void pgc_slots_of_bin(uint32_t A, uint32_t bin, uint32_t* sa, uint32_t* sb) {
    uint32_t a = 0, rest = bin;
    while (a + 1 < A && rest >= A - a) { rest -= A - a; ++a; }
    *sa = a;
    *sb = a + rest;
}
