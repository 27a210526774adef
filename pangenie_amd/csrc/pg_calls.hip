// pg_calls.hip — genotype calls on the device (gfx950): GT and GQ per variant from the finished bins, DESIGN.md §4e.
//
// What the host does per variant in long double — GenotypingResult::normalize, get_likeliest_genotype and
// get_genotype_quality (reference src/genotypingresult.cpp:118-210) — done here in the integer pairs of pg_calls.h,
// which give the long double's bits.  One 8-byte record per variant leaves the device instead of 12 bytes per bin.
//
//   k_calls       one lane per variant, variants with at most PG_AMAX alleles (15 bins); no LDS, no atomics, and the bins
//                 are walked three times rather than kept (an array indexed at run time would be scratch memory)
//   k_calls_wide  one wave per listed variant with more alleles: the sum in bin order by every lane alike (rounded
//                 additions do not associate: no tree), the divisions and the maximum spread over the lanes
// One launch of each covers every chain of a job: a descriptor per chain, a block finds its chain by bisection.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_calls.h"
#include "pg_calls_dev.h"
#include "pg_launch.h"

#define PC_BLOCK 256
#define PC_WAVES (PC_BLOCK / 64)

namespace {

// the last descriptor whose first block is <= b (descriptors of chains without variants are not in the list)
__device__ __forceinline__ uint32_t calls_chain_of(const CallsDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the keys of a narrow variant in map order: allele slots a <= b, both present
struct NarrowKeys {
    const double* lik;        // the variant's first bin
    const int32_t* lik_exp;
    uint32_t A, present;      // bit a: allele slot a occurs on a selected path (0 for a variant that is not kept)
    uint32_t a, b, bin;
    __device__ void start() { a = 0; b = 0; bin = 0; }
    __device__ bool next(pgx* v) {
        while (a < A) {
            const uint32_t ca = a, cb = b, cbin = bin;
            ++bin;
            if (++b == A) { ++a; b = a; }
            if (((present >> ca) & (present >> cb)) & 1u) {
                *v = pgx_from_bin(lik[cbin], lik_exp[cbin]);
                return true;
            }
        }
        return false;
    }
    // allele slots of key number k
    __device__ void locate(uint32_t k, uint32_t* sa, uint32_t* sb) const {
        uint32_t n = 0;
        *sa = 0; *sb = 0;
        for (uint32_t x = 0; x < A; ++x)
            for (uint32_t y = x; y < A; ++y)
                if (((present >> x) & (present >> y)) & 1u) {
                    if (n == k) { *sa = x; *sb = y; }
                    ++n;
                }
    }
};

__global__ __launch_bounds__(PC_BLOCK) void k_calls(const DevContig* __restrict__ contigs, const CallsDesc* __restrict__ desc, uint32_t n_desc,
                                                    const uint64_t* __restrict__ thr_m, const int32_t* __restrict__ thr_e) {
    const uint32_t blk = blockIdx.x;
    const CallsDesc cd = desc[calls_chain_of(desc, n_desc, blk)];
    const uint32_t v = (blk - cd.blk0) * PC_BLOCK + threadIdx.x;
    if (v >= cd.V) return;
    const DevContig* __restrict__ c = contigs + cd.chain;
    const uint32_t a0 = c->allele_off[v];
    const uint32_t A = c->allele_off[v + 1] - a0;
    if (A > PG_AMAX) return;   // k_calls_wide's
    unsigned long long* __restrict__ out = (unsigned long long*)cd.out;
    uint32_t present = 0;
    if (c->kept[v])
        for (uint32_t a = 0; a < A; ++a) present |= (c->allele_present[a0 + a] ? 1u : 0u) << a;
    const uint64_t g0 = c->geno_off[v];
    NarrowKeys keys;
    keys.lik = c->lik + g0;
    keys.lik_exp = c->lik_exp + g0;
    keys.A = A;
    keys.present = present;
    const pgx_decision r = pgx_decide(keys, thr_m, thr_e);
    unsigned long long rec = pack_no_call(r.flags);
    if (r.flags == PGX_CALL_OK) {
        uint32_t sa, sb;
        keys.locate(r.best, &sa, &sb);
        rec = pack_call(c->allele_id[a0 + sa], c->allele_id[a0 + sb], r.gq, PGX_CALL_OK);
    }
    out[v] = rec;
}

__global__ __launch_bounds__(PC_BLOCK) void k_calls_wide(const DevContig* __restrict__ contigs, const CallsDesc* __restrict__ desc,
                                                         const uint2* __restrict__ list, uint32_t n_list,
                                                         const uint64_t* __restrict__ thr_m, const int32_t* __restrict__ thr_e) {
    const uint32_t entry = blockIdx.x * PC_WAVES + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (entry >= n_list) return;   // (whole waves leave)
    const uint2 e = list[entry];   // {descriptor, variant}
    const CallsDesc cd = desc[e.x];
    const uint32_t v = e.y;
    const DevContig* __restrict__ c = contigs + cd.chain;
    unsigned long long* __restrict__ out = (unsigned long long*)cd.out;
    const uint32_t a0 = c->allele_off[v];
    const uint32_t A = c->allele_off[v + 1] - a0;
    const uint8_t* __restrict__ pres = c->allele_present + a0;
    const uint64_t g0 = c->geno_off[v];
    const double* __restrict__ lik = c->lik + g0;
    const int32_t* __restrict__ lik_exp = c->lik_exp + g0;
    if (!c->kept[v]) {
        if (lane == 0) out[v] = pack_no_call(PGX_CALL_NONE);
        return;
    }
    // the sum, key after key in the map's order, by every lane alike
    pgx sum = pgx_zero(), largest = pgx_zero();
    {
        uint32_t bin = 0;
        for (uint32_t a = 0; a < A; ++a) {
            if (!pres[a]) { bin += A - a; continue; }
            for (uint32_t b = a; b < A; ++b, ++bin) {
                if (!pres[b]) continue;
                const pgx x = pgx_from_bin(lik[bin], lik_exp[bin]);
                sum = pgx_add(sum, x);
                if (pgx_cmp(x, largest) > 0) largest = x;
            }
        }
    }
    if (sum.m == 0 || pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) {
        if (lane == 0) out[v] = pack_no_call(sum.m == 0 ? PGX_CALL_NONE : PGX_CALL_DEFERRED);
        return;
    }
    // the likeliest genotype: lane l takes the keys (a, a + l), (a, a + l + 64), ... of every row a
    pgx best = pgx_zero();
    uint32_t best_bin = 0;
    {
        uint32_t row = 0;   // first bin of row a
        for (uint32_t a = 0; a < A; ++a) {
            if (pres[a])
                for (uint32_t b = a + lane; b < A; b += 64u) {
                    if (!pres[b]) continue;
                    const uint32_t bin = row + (b - a);
                    const pgx q = pgx_div(pgx_from_bin(lik[bin], lik_exp[bin]), sum);
                    if (wide_better(q, bin, best, best_bin)) { best = q; best_bin = bin; }
                }
            row += A - a;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        pgx o;
        o.m = __shfl_xor((unsigned long long)best.m, m, 64);
        o.e = __shfl_xor(best.e, m, 64);
        const uint32_t o_bin = __shfl_xor(best_bin, m, 64);
        if (wide_better(o, o_bin, best, best_bin)) { best = o; best_bin = o_bin; }
    }
    // a unique maximum?
    bool tie = false;
    {
        uint32_t row = 0;
        for (uint32_t a = 0; a < A; ++a) {
            if (pres[a])
                for (uint32_t b = a + lane; b < A; b += 64u) {
                    const uint32_t bin = row + (b - a);
                    if (!pres[b] || bin == best_bin) continue;
                    if (pgx_within_tie(best, pgx_div(pgx_from_bin(lik[bin], lik_exp[bin]), sum))) tie = true;
                }
            row += A - a;
        }
    }
    const bool any_tie = __ballot(tie ? 1 : 0) != 0ull;
    if (lane != 0) return;
    if (any_tie) { out[v] = pack_no_call(PGX_CALL_NOT_UNIQUE); return; }
    uint32_t sa = 0, rest = best_bin;
    while (sa + 1 < A && rest >= A - sa) { rest -= A - sa; ++sa; }
    const uint32_t sb = sa + rest;   // (< A: best_bin is a bin of the variant)
    out[v] = pack_call(c->allele_id[a0 + sa], c->allele_id[a0 + sb], pgx_gq_of_best(best, thr_m, thr_e), PGX_CALL_OK);
}

// ---------------------------------------------------------------------------------------------------------------
//  Calls per VCF RECORD (DESIGN.md 4e "Records"): a bubble merged from several records is folded onto each record's own
//  alleles, the genotypes over undefined alleles are dropped and the rest renormalised, then GT and GQ as above.
//
//   k_rcalls       one lane per record of a bubble with at most PG_AMAX alleles: pgx_decide_record (pg_calls.h) walks the
//                  bubble's at most 15 keys once per key of the folded map; the record alleles of the (at most five)
//                  slots ride in one 64-bit register, a byte each (a record has at most 256 alleles)
//   k_rcalls_wide  one wave (= one block) per listed record of a wider bubble.  The bubble's sum in bin order by every
//                  lane alike; the quotients spread over the lanes into the wave's staging slot Q; the keys of the folded
//                  map dealt to the lanes (lane l: keys l, l + 64, ...), each added up in the bubble's order into F; the
//                  renormalising sum over F in key order by every lane alike; best and runner-up by shuffle.
//                  A key nothing folds onto reads 0 here instead of being absent: it cannot win `>=` against a positive
//                  best and cannot tie with one (the best of at most 32 896 values that add up to 1 is far above 1e-10).
// ---------------------------------------------------------------------------------------------------------------
#define PCW_BLOCK 64

struct NarrowRecordKeys {
    const double* lik;
    const int32_t* lik_exp;
    uint32_t A, present;
    unsigned long long own;   // byte s: the record allele of slot s
    uint32_t a, b, bin;
    __device__ void start() { a = 0; b = 0; bin = 0; }
    __device__ bool next(pgx* v, uint32_t* key) {
        while (a < A) {
            const uint32_t ca = a, cb = b, cbin = bin;
            ++bin;
            if (++b == A) { ++a; b = a; }
            if (((present >> ca) & (present >> cb)) & 1u) {
                const uint32_t oa = (uint32_t)(own >> (8u * ca)) & 0xFFu, ob = (uint32_t)(own >> (8u * cb)) & 0xFFu;
                *v = pgx_from_bin(lik[cbin], lik_exp[cbin]);
                *key = oa <= ob ? (oa << 16) | ob : (ob << 16) | oa;
                return true;
            }
        }
        return false;
    }
};

struct DefinedAllele {
    const uint16_t* vcf;   // the record's vcf_index
    __device__ bool operator()(uint32_t a) const { return vcf[a] != 0xFFFFu; }
};

__device__ __forceinline__ uint32_t rcalls_chain_of(const RCallsDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PC_BLOCK) void k_rcalls(const DevContig* __restrict__ contigs, const RCallsDesc* __restrict__ desc, uint32_t n_desc,
                                                     const uint64_t* __restrict__ thr_m, const int32_t* __restrict__ thr_e) {
    const uint32_t blk = blockIdx.x;
    const RCallsDesc* __restrict__ cd = desc + rcalls_chain_of(desc, n_desc, blk);
    const uint32_t r = (blk - cd->blk0) * PC_BLOCK + threadIdx.x;
    if (r >= cd->R) return;
    const DevContig* __restrict__ c = contigs + cd->chain;
    const uint32_t rv = cd->plan.rec_var[r], v = rv & 0x7FFFFFFFu;
    const uint32_t a0 = c->allele_off[v];
    const uint32_t A = c->allele_off[v + 1] - a0;
    if (A > PG_AMAX) return;   // k_rcalls_wide's
    const uint32_t m0 = cd->plan.map_off[r], n_map = cd->plan.map_off[r + 1] - m0;
    const uint16_t* __restrict__ map = cd->plan.map + m0;
    uint32_t present = 0;
    unsigned long long own = 0;
    if (c->kept[v])
        for (uint32_t a = 0; a < A; ++a)
            if (c->allele_present[a0 + a]) {
                present |= 1u << a;
                const uint32_t id = c->allele_id[a0 + a];   // (k_rplan_ids has checked id < n_map; no read outside the map either way)
                own |= (unsigned long long)(id < n_map ? map[id] & 0xFFu : 0u) << (8u * a);
            }
    const uint64_t g0 = c->geno_off[v];
    NarrowRecordKeys keys;
    keys.lik = c->lik + g0;
    keys.lik_exp = c->lik_exp + g0;
    keys.A = A;
    keys.present = present;
    keys.own = own;
    DefinedAllele def;
    def.vcf = cd->plan.vcf_index + cd->plan.vcf_off[r];
    const pgx_record_decision d = pgx_decide_record(keys, (rv >> 31) != 0u, def, thr_m, thr_e);
    unsigned long long rec = pack_no_call(d.flags);
    if ((d.flags & 0xFFu) == PGX_CALL_OK) rec = pack_call(def.vcf[d.key >> 16], def.vcf[d.key & 0xFFFFu], d.gq, d.flags);
    ((unsigned long long*)cd->out)[r] = rec;
}

// The id check of the record plans: one lane per record of every chain that has a plan, over k_rcalls'
// descriptors.  Record r of bubble v holds every allele id of v against the length of its map; a lane that finds one
// outside it leaves (chain << 32 | v) in *hit if that is lower than what is there (the host reads the lowest pair and names
// it).  The ids of a sampled panel exist on the device alone; k_rcalls' clamp stays whatever this finds.
__global__ __launch_bounds__(PC_BLOCK) void k_rplan_ids(const DevContig* __restrict__ contigs, const RCallsDesc* __restrict__ desc, uint32_t n_desc,
                                                        unsigned long long* __restrict__ hit) {
    const uint32_t blk = blockIdx.x;
    const RCallsDesc* __restrict__ cd = desc + rcalls_chain_of(desc, n_desc, blk);
    const uint32_t r = (blk - cd->blk0) * PC_BLOCK + threadIdx.x;
    if (r >= cd->R) return;
    const DevContig* __restrict__ c = contigs + cd->chain;
    const uint32_t v = cd->plan.rec_var[r] & 0x7FFFFFFFu;
    const uint32_t a0 = c->allele_off[v], a1 = c->allele_off[v + 1];
    const uint32_t n_map = cd->plan.map_off[r + 1] - cd->plan.map_off[r];
    bool outside = false;
    for (uint32_t a = a0; a < a1; ++a) outside = outside || c->allele_id[a] >= n_map;
    if (outside) atomicMin(hit, ((unsigned long long)cd->chain << 32) | v);
}

struct PgxSlot {   // a staged value: 16 bytes
    unsigned long long m;
    int32_t e, pad;
};
__device__ __forceinline__ pgx slot_get(const PgxSlot* s) { pgx r; r.m = s->m; r.e = s->e; return r; }
__device__ __forceinline__ void slot_put(PgxSlot* s, pgx x) { s->m = x.m; s->e = x.e; }

// (value, key) of two lanes' bests: the later key of equal values wins, a lane without keys never does
__device__ __forceinline__ bool top2_other_wins(const pgx_top2& mine, pgx o_best, unsigned long long o_key) {
    if (o_key == PGX_NO_KEY) return false;
    if (mine.best_key == PGX_NO_KEY) return true;
    const int c = pgx_cmp(o_best, mine.best);
    return c > 0 || (c == 0 && o_key > mine.best_key);
}

__global__ __launch_bounds__(PCW_BLOCK) void k_rcalls_wide(const DevContig* __restrict__ contigs, const RCallsDesc* __restrict__ desc,
                                                           const uint2* __restrict__ list, uint32_t n_list, PgxSlot* __restrict__ stage,
                                                           uint32_t max_bins, uint32_t stride, const uint64_t* __restrict__ thr_m,
                                                           const int32_t* __restrict__ thr_e) {
    __shared__ uint16_t s_own[PG_MAX_ALLELES_PER_VARIANT];   // per slot: its record allele; 0xFFFF: not on a selected path (or not a kept column)
    const uint32_t lane = threadIdx.x;
    PgxSlot* __restrict__ Q = stage + (size_t)blockIdx.x * stride;   // [max_bins] the bubble's quotients
    PgxSlot* __restrict__ F = Q + max_bins;                          // [stride - max_bins] the folded map
    for (uint32_t entry = blockIdx.x; entry < n_list; entry += gridDim.x) {
        __syncthreads();   // the previous record's s_own, Q and F are done with
        const uint2 e = list[entry];   // {descriptor, record}
        const RCallsDesc* __restrict__ cd = desc + e.x;
        const uint32_t r = e.y;
        const DevContig* __restrict__ c = contigs + cd->chain;
        unsigned long long* __restrict__ out = (unsigned long long*)cd->out;
        const uint32_t rv = cd->plan.rec_var[r], v = rv & 0x7FFFFFFFu;
        const bool undef = (rv >> 31) != 0u;
        const uint32_t a0 = c->allele_off[v];
        const uint32_t A = c->allele_off[v + 1] - a0;
        const uint32_t m0 = cd->plan.map_off[r], n_map = cd->plan.map_off[r + 1] - m0;
        const uint16_t* __restrict__ map = cd->plan.map + m0;
        const uint32_t vcf0 = cd->plan.vcf_off[r], nA = cd->plan.vcf_off[r + 1] - vcf0;
        const uint16_t* __restrict__ vcf = cd->plan.vcf_index + vcf0;
        const uint32_t K = nA * (nA + 1u) / 2u;
        const uint64_t g0 = c->geno_off[v];
        const double* __restrict__ lik = c->lik + g0;
        const int32_t* __restrict__ lik_exp = c->lik_exp + g0;
        const bool kept = c->kept[v] != 0;
        for (uint32_t a = lane; a < A; a += PCW_BLOCK) {
            const uint32_t id = c->allele_id[a0 + a];   // (k_rplan_ids has checked id < n_map; no read outside the map either way)
            s_own[a] = (kept && c->allele_present[a0 + a]) ? (id < n_map ? map[id] : (uint16_t)0u) : (uint16_t)0xFFFFu;
        }
        __syncthreads();
        // the bubble's sum, key after key in the map's order, by every lane alike
        pgx sum = pgx_zero(), largest = pgx_zero();
        uint32_t n_keys = 0;
        {
            uint32_t bin = 0;
            for (uint32_t a = 0; a < A; ++a) {
                if (s_own[a] == 0xFFFFu) { bin += A - a; continue; }
                for (uint32_t b = a; b < A; ++b, ++bin) {
                    if (s_own[b] == 0xFFFFu) continue;
                    const pgx x = pgx_from_bin(lik[bin], lik_exp[bin]);
                    sum = pgx_add(sum, x);
                    if (pgx_cmp(x, largest) > 0) largest = x;
                    ++n_keys;
                }
            }
        }
        if (n_keys == 0 || sum.m == 0 || pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) {   // (the same on every lane)
            if (lane == 0)
                out[r] = n_keys == 0 ? pack_call(0u, 0u, PG_GQ_CERTAIN, PGX_CALL_OK | PGX_CALL_EMPTY)
                                     : pack_no_call(sum.m == 0 ? PGX_CALL_NONE : PGX_CALL_DEFERRED);
            continue;
        }
        // the quotients: lane l takes the keys (a, a + l), (a, a + l + 64), ... of every row a
        {
            uint32_t row = 0;
            for (uint32_t a = 0; a < A; ++a) {
                if (s_own[a] != 0xFFFFu)
                    for (uint32_t b = a + lane; b < A; b += PCW_BLOCK) {
                        if (s_own[b] == 0xFFFFu) continue;
                        const uint32_t bin = row + (b - a);
                        slot_put(Q + bin, pgx_div(pgx_from_bin(lik[bin], lik_exp[bin]), sum));
                    }
                row += A - a;
            }
        }
        __syncthreads();
        // the fold: key (ra, rb) receives the keys (a, b) whose slots carry ra and rb, in the bubble's order
        for (uint32_t k = lane; k < K; k += PCW_BLOCK) {
            uint32_t ra = 0, rest = k;
            while (rest >= nA - ra) { rest -= nA - ra; ++ra; }
            const uint32_t rb = ra + rest;
            pgx acc = pgx_zero();
            uint32_t row = 0;
            for (uint32_t a = 0; a < A; ++a) {
                const uint32_t oa = s_own[a];
                if (oa == ra || oa == rb) {
                    const uint32_t other = oa == ra ? rb : ra;
                    for (uint32_t b = a; b < A; ++b)
                        if (s_own[b] == other) acc = pgx_add(acc, slot_get(Q + row + (b - a)));
                }
                row += A - a;
            }
            slot_put(F + k, acc);
        }
        __syncthreads();
        // get_specific_likelihoods: the defined keys of F added in key order, by every lane alike
        pgx sum2 = pgx_zero();
        if (undef) {
            uint32_t k = 0;
            for (uint32_t ra = 0; ra < nA; ++ra) {
                if (vcf[ra] == 0xFFFFu) { k += nA - ra; continue; }
                for (uint32_t rb = ra; rb < nA; ++rb, ++k)
                    if (vcf[rb] != 0xFFFFu) sum2 = pgx_add(sum2, slot_get(F + k));
            }
            if (sum2.m == 0) {
                if (lane == 0) out[r] = pack_no_call(PGX_CALL_NONE);
                continue;
            }
        }
        // the likeliest genotype and the runner-up
        pgx_top2 t;
        pgx_top2_init(&t);
        for (uint32_t k = lane; k < K; k += PCW_BLOCK) {
            uint32_t ra = 0, rest = k;
            while (rest >= nA - ra) { rest -= nA - ra; ++ra; }
            const uint32_t rb = ra + rest;
            if (undef && (vcf[ra] == 0xFFFFu || vcf[rb] == 0xFFFFu)) continue;
            pgx f = slot_get(F + k);
            if (undef) f = pgx_div(f, sum2);
            pgx_top2_take(&t, f, ((unsigned long long)ra << 16) | rb);
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            pgx ob, os;
            ob.m = __shfl_xor((unsigned long long)t.best.m, m, 64);
            ob.e = __shfl_xor(t.best.e, m, 64);
            os.m = __shfl_xor((unsigned long long)t.second.m, m, 64);
            os.e = __shfl_xor(t.second.e, m, 64);
            const unsigned long long o_key = __shfl_xor((unsigned long long)t.best_key, m, 64);
            const bool o_has_second = __shfl_xor(t.has_second ? 1 : 0, m, 64) != 0;
            // the loser's best is a candidate for the runner-up, as is the other lane's own runner-up
            pgx cand = ob;
            bool has_cand = o_key != PGX_NO_KEY;
            if (top2_other_wins(t, ob, o_key)) {
                cand = t.best;
                has_cand = t.best_key != PGX_NO_KEY;
                t.best = ob;
                t.best_key = o_key;
            }
            if (has_cand && (!t.has_second || pgx_cmp(cand, t.second) > 0)) { t.second = cand; t.has_second = true; }
            if (o_has_second && (!t.has_second || pgx_cmp(os, t.second) > 0)) { t.second = os; t.has_second = true; }
        }
        if (lane != 0) continue;
        unsigned long long rec;
        if (t.best.m == 0) rec = pack_no_call(PGX_CALL_NONE);
        else if (t.has_second && pgx_within_tie(t.best, t.second)) rec = pack_no_call(PGX_CALL_NOT_UNIQUE);
        else rec = pack_call(vcf[(uint32_t)(t.best_key >> 16)], vcf[(uint32_t)(t.best_key & 0xFFFFu)], pgx_gq_of_best(t.best, thr_m, thr_e), PGX_CALL_OK);
        out[r] = rec;
    }
}

// ---------------------------------------------------------------------------------------------------------------
//  The GL column per VCF record: log10 of every genotype's likelihood over the record's defined alleles, as
//  the four digits the VCF prints (pg_gl, 4 bytes).  The likelihoods are those of the record calls — the same key iterator,
//  slot packing and staging — and pgx_gl (pg_calls.h) turns each into its digits or leaves it to the host (PG_GL_DEFERRED).
//
//   k_rgl        one lane per record of a bubble with at most PG_AMAX alleles: pgx_record_gl walks the bubble's keys once per
//                defined genotype pair of the record (twice for a record with undefined alleles: first for sum2)
//   k_rgl_wide   one wave (= one block) per listed record of a wider bubble: quotients and then the folded map in the block's
//                staging slot as in k_rcalls_wide, sum2 in key order by every lane alike, lane l converts keys l, l + 64, ...
//   k_gl_values  one lane per (m, e) pair: the unit entry that puts the device's own log10 / log1p under test
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gl_word(pg_gl g) { return (uint32_t)(uint16_t)g.mant | ((uint32_t)(uint16_t)g.exp10 << 16); }

struct VcfIndexOf {
    const uint16_t* vcf;   // the record's vcf_index
    __device__ uint32_t operator()(uint32_t a) const { return vcf[a]; }
};
struct GlStore {
    uint32_t* out;         // the record's values
    __device__ void operator()(uint32_t i, pg_gl g) const { out[i] = gl_word(g); }
};

__device__ __forceinline__ uint32_t rgl_chain_of(const RGlDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PC_BLOCK) void k_rgl(const DevContig* __restrict__ contigs, const RGlDesc* __restrict__ desc, uint32_t n_desc) {
    const uint32_t blk = blockIdx.x;
    const RGlDesc* __restrict__ cd = desc + rgl_chain_of(desc, n_desc, blk);
    const uint32_t r = (blk - cd->blk0) * PC_BLOCK + threadIdx.x;
    if (r >= cd->R) return;
    const DevContig* __restrict__ c = contigs + cd->chain;
    const uint32_t rv = cd->plan.rec_var[r], v = rv & 0x7FFFFFFFu;
    const uint32_t a0 = c->allele_off[v];
    const uint32_t A = c->allele_off[v + 1] - a0;
    if (A > PG_AMAX) return;   // k_rgl_wide's
    const uint32_t m0 = cd->plan.map_off[r], n_map = cd->plan.map_off[r + 1] - m0;
    const uint16_t* __restrict__ map = cd->plan.map + m0;
    uint32_t present = 0;
    unsigned long long own = 0;
    if (c->kept[v])
        for (uint32_t a = 0; a < A; ++a)
            if (c->allele_present[a0 + a]) {
                present |= 1u << a;
                const uint32_t id = c->allele_id[a0 + a];   // (k_rplan_ids has checked id < n_map; no read outside the map either way)
                own |= (unsigned long long)(id < n_map ? map[id] & 0xFFu : 0u) << (8u * a);
            }
    const uint64_t g0 = c->geno_off[v];
    NarrowRecordKeys keys;
    keys.lik = c->lik + g0;
    keys.lik_exp = c->lik_exp + g0;
    keys.A = A;
    keys.present = present;
    keys.own = own;
    const uint32_t vcf0 = cd->plan.vcf_off[r];
    VcfIndexOf vcf;
    vcf.vcf = cd->plan.vcf_index + vcf0;
    GlStore store;
    store.out = (uint32_t*)cd->out + cd->gl_off[r];
    pgx_record_gl(keys, cd->plan.vcf_off[r + 1] - vcf0, (rv >> 31) != 0u, vcf, store);
}

__global__ __launch_bounds__(PCW_BLOCK) void k_rgl_wide(const DevContig* __restrict__ contigs, const RGlDesc* __restrict__ desc,
                                                        const uint2* __restrict__ list, uint32_t n_list, PgxSlot* __restrict__ stage,
                                                        uint32_t max_bins, uint32_t stride) {
    __shared__ uint16_t s_own[PG_MAX_ALLELES_PER_VARIANT];   // per slot: its record allele; 0xFFFF: not on a selected path (or not a kept column)
    const uint32_t lane = threadIdx.x;
    PgxSlot* __restrict__ Q = stage + (size_t)blockIdx.x * stride;   // [max_bins] the bubble's quotients
    PgxSlot* __restrict__ F = Q + max_bins;                          // [stride - max_bins] the folded map
    for (uint32_t entry = blockIdx.x; entry < n_list; entry += gridDim.x) {
        __syncthreads();   // the previous record's s_own, Q and F are done with
        const uint2 e = list[entry];   // {descriptor, record}
        const RGlDesc* __restrict__ cd = desc + e.x;
        const uint32_t r = e.y;
        const DevContig* __restrict__ c = contigs + cd->chain;
        uint32_t* __restrict__ out = (uint32_t*)cd->out + cd->gl_off[r];
        const uint32_t rv = cd->plan.rec_var[r], v = rv & 0x7FFFFFFFu;
        const bool undef = (rv >> 31) != 0u;
        const uint32_t a0 = c->allele_off[v];
        const uint32_t A = c->allele_off[v + 1] - a0;
        const uint32_t m0 = cd->plan.map_off[r], n_map = cd->plan.map_off[r + 1] - m0;
        const uint16_t* __restrict__ map = cd->plan.map + m0;
        const uint32_t vcf0 = cd->plan.vcf_off[r], nA = cd->plan.vcf_off[r + 1] - vcf0;
        const uint16_t* __restrict__ vcf = cd->plan.vcf_index + vcf0;
        const uint32_t K = nA * (nA + 1u) / 2u;
        const uint64_t g0 = c->geno_off[v];
        const double* __restrict__ lik = c->lik + g0;
        const int32_t* __restrict__ lik_exp = c->lik_exp + g0;
        const bool kept = c->kept[v] != 0;
        for (uint32_t a = lane; a < A; a += PCW_BLOCK) {
            const uint32_t id = c->allele_id[a0 + a];   // (k_rplan_ids has checked id < n_map; no read outside the map either way)
            s_own[a] = (kept && c->allele_present[a0 + a]) ? (id < n_map ? map[id] : (uint16_t)0u) : (uint16_t)0xFFFFu;
        }
        __syncthreads();
        uint32_t nd = 0;
        for (uint32_t a = 0; a < nA; ++a) nd += vcf[a] != 0xFFFFu ? 1u : 0u;
        const uint32_t n_values = nd * (nd + 1u) / 2u;
        // the bubble's sum, key after key in the map's order, by every lane alike
        pgx sum = pgx_zero(), largest = pgx_zero();
        uint32_t n_keys = 0;
        {
            uint32_t bin = 0;
            for (uint32_t a = 0; a < A; ++a) {
                if (s_own[a] == 0xFFFFu) { bin += A - a; continue; }
                for (uint32_t b = a; b < A; ++b, ++bin) {
                    if (s_own[b] == 0xFFFFu) continue;
                    const pgx x = pgx_from_bin(lik[bin], lik_exp[bin]);
                    sum = pgx_add(sum, x);
                    if (pgx_cmp(x, largest) > 0) largest = x;
                    ++n_keys;
                }
            }
        }
        if (n_keys == 0 || sum.m == 0 || pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) {   // (the same on every lane)
            const uint32_t g = gl_word((n_keys == 0 || sum.m == 0) ? pgx_gl_neg_inf() : pgx_gl_deferred());
            for (uint32_t i = lane; i < n_values; i += PCW_BLOCK) out[i] = (n_keys == 0 && i == 0) ? gl_word(pgx_gl_of(0, 0)) : g;
            continue;
        }
        // the quotients: lane l takes the keys (a, a + l), (a, a + l + 64), ... of every row a
        {
            uint32_t row = 0;
            for (uint32_t a = 0; a < A; ++a) {
                if (s_own[a] != 0xFFFFu)
                    for (uint32_t b = a + lane; b < A; b += PCW_BLOCK) {
                        if (s_own[b] == 0xFFFFu) continue;
                        const uint32_t bin = row + (b - a);
                        slot_put(Q + bin, pgx_div(pgx_from_bin(lik[bin], lik_exp[bin]), sum));
                    }
                row += A - a;
            }
        }
        __syncthreads();
        // the fold: key (ra, rb) receives the keys (a, b) whose slots carry ra and rb, in the bubble's order
        for (uint32_t k = lane; k < K; k += PCW_BLOCK) {
            uint32_t ra = 0, rest = k;
            while (rest >= nA - ra) { rest -= nA - ra; ++ra; }
            const uint32_t rb = ra + rest;
            pgx acc = pgx_zero();
            uint32_t row = 0;
            for (uint32_t a = 0; a < A; ++a) {
                const uint32_t oa = s_own[a];
                if (oa == ra || oa == rb) {
                    const uint32_t other = oa == ra ? rb : ra;
                    for (uint32_t b = a; b < A; ++b)
                        if (s_own[b] == other) acc = pgx_add(acc, slot_get(Q + row + (b - a)));
                }
                row += A - a;
            }
            slot_put(F + k, acc);
        }
        __syncthreads();
        // get_specific_likelihoods: the defined keys of F added in key order, by every lane alike
        pgx sum2 = pgx_zero();
        if (undef) {
            uint32_t k = 0;
            for (uint32_t ra = 0; ra < nA; ++ra) {
                if (vcf[ra] == 0xFFFFu) { k += nA - ra; continue; }
                for (uint32_t rb = ra; rb < nA; ++rb, ++k)
                    if (vcf[rb] != 0xFFFFu) sum2 = pgx_add(sum2, slot_get(F + k));
            }
        }
        // the digits: lane l converts and stores the keys l, l + 64, ...
        for (uint32_t k = lane; k < K; k += PCW_BLOCK) {
            uint32_t ra = 0, rest = k;
            while (rest >= nA - ra) { rest -= nA - ra; ++ra; }
            const uint32_t va = vcf[ra], vb = vcf[ra + rest];
            if (va == 0xFFFFu || vb == 0xFFFFu) continue;
            pgx f = slot_get(F + k);
            if (sum2.m != 0) f = pgx_div(f, sum2);
            out[vb * (vb + 1u) / 2u + va] = gl_word(pgx_gl(f));
        }
    }
}

__global__ __launch_bounds__(PC_BLOCK) void k_gl_values(const uint64_t* __restrict__ m, const int32_t* __restrict__ e, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= n) return;
    pgx x;
    x.m = m[i];
    x.e = e[i];
    out[i] = gl_word(pgx_gl(x));
}

}  // namespace

extern "C" void pgk_launch_rgl(const DevContig* d_contigs, const RGlDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                               void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_rgl, dim3(n_blocks), dim3(PC_BLOCK), 0, s, d_contigs, d_desc, n_desc);
    if (n_wide && n_slots)
        hipLaunchKernelGGL(k_rgl_wide, dim3(n_slots < n_wide ? n_slots : n_wide), dim3(PCW_BLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, n_wide,
                           (PgxSlot*)d_stage, max_bins, stride);
}

extern "C" void pgk_launch_gl_values(const uint64_t* d_m, const int32_t* d_e, void* d_out, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_gl_values, dim3((n + PC_BLOCK - 1) / PC_BLOCK), dim3(PC_BLOCK), 0, s, d_m, d_e, (uint32_t*)d_out, n);
}

extern "C" void pgk_launch_rcalls(const DevContig* d_contigs, const RCallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide,
                                  uint32_t n_wide, void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, const uint64_t* d_thr_m,
                                  const int32_t* d_thr_e, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_rcalls, dim3(n_blocks), dim3(PC_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_thr_m, d_thr_e);
    if (n_wide && n_slots)
        hipLaunchKernelGGL(k_rcalls_wide, dim3(n_slots < n_wide ? n_slots : n_wide), dim3(PCW_BLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, n_wide,
                           (PgxSlot*)d_stage, max_bins, stride, d_thr_m, d_thr_e);
}

extern "C" void pgk_launch_rplan_ids(const DevContig* d_contigs, const RCallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, void* d_hit, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_rplan_ids, dim3(n_blocks), dim3(PC_BLOCK), 0, s, d_contigs, d_desc, n_desc, (unsigned long long*)d_hit);
}

extern "C" void pgk_launch_calls(const DevContig* d_contigs, const CallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide,
                                 uint32_t n_wide, const uint64_t* d_thr_m, const int32_t* d_thr_e, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_calls, dim3(n_blocks), dim3(PC_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_thr_m, d_thr_e);
    if (n_wide)
        hipLaunchKernelGGL(k_calls_wide, dim3((n_wide + PC_WAVES - 1) / PC_WAVES), dim3(PC_BLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, n_wide,
                           d_thr_m, d_thr_e);
}
extern "C" uint32_t pgk_calls_block(void) { return PC_BLOCK; }
