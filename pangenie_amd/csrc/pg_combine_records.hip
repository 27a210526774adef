// pg_combine_records.hip — path subsets to VCF lines on the device (gfx950): GT, GQ and the GL column per VCF RECORD from a
// group's combined bins.  DESIGN.md §4e-5.
//
// What Graph::write_genotypes does per record of a bubble on the combined map — normalize, Variant::separate_variants,
// get_specific_likelihoods, likeliest genotype, quality, log10 — in the integer pairs of pg_calls.h, with the functions the
// record calls and record GLs of ONE chain use (pgx_decide_record, pgx_record_gl, pgx_gl).  Only the key source differs:
// the keys of a bubble are its combined bins with PG_COMBINED_PRESENT (pg_combine.h), not the pairs of present alleles.
//
//   k_crcalls       one lane per record of a bubble with at most PG_AMAX alleles: pgx_decide_record over pgc_record_keys
//   k_crgl          the same walk through pgx_record_gl
//   k_crcalls_wide  one wave (= one block) per listed record of a wider bubble, the structure of k_rcalls_wide: the sum in bin
//   k_crgl_wide     order by every lane alike; quotients spread over the lanes into the block's staging slot; the folded map
//                   dealt to the lanes; sum2 in key order by every lane alike; then best and runner-up by shuffle / the digits
//   k_crplan_ids    the allele ids of a group's first chain against the maps of its plan
// A variant with a PG_COMBINED_DEFERRED bin leaves every record and every value to the host.
// One launch of each covers every group of a job: a descriptor per group, a block finds its group by bisection.
// No scratch; the one atomic is k_crplan_ids' atomicMin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_calls_dev.h"
#include "pg_combine.h"
#include "pg_launch.h"

#define PCR_BLOCK 256
#define PCR_WBLOCK 64

static_assert(PG_AMAX <= 8, "pgc_own_packed carries the record alleles of a narrow bubble's slots a byte each in 64 bits");

namespace {

// the last descriptor whose first block is <= b (groups without records are not in the list)
__device__ __forceinline__ uint32_t crec_group_of(const CRecDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t gl_word(pg_gl g) { return (uint32_t)(uint16_t)g.mant | ((uint32_t)(uint16_t)g.exp10 << 16); }

struct DefinedAllele {
    const uint16_t* vcf;   // the record's vcf_index
    __device__ bool operator()(uint32_t a) const { return vcf[a] != 0xFFFFu; }
};
// (both keep what is the same for every lane of a block apart from the lane's own 32-bit index: a register less each across pgx_gl)
struct VcfIndexOf {
    const uint16_t* vcf;   // the plan's vcf_index
    uint32_t at;           // the record's first entry
    __device__ uint32_t operator()(uint32_t a) const { return vcf[at + a]; }
};
struct GlStore {
    const CRecDesc* cd;
    uint32_t r;            // value i of record r lies at gl[gl_off[r] + i]
    __device__ void operator()(uint32_t i, pg_gl g) const { ((uint32_t*)cd->gl)[cd->gl_off[r] + i] = gl_word(g); }
};

// record r of a narrow bubble: its keys; false: the bubble is a wide kernel's
__device__ __forceinline__ bool narrow_keys(const DevContig* __restrict__ c, const CRecDesc* __restrict__ cd, uint32_t r, pgc_record_keys* keys) {
    const uint32_t v = cd->plan.rec_var[r] & 0x7FFFFFFFu;
    const uint32_t a0 = c->allele_off[v];
    const uint32_t A = c->allele_off[v + 1] - a0;
    if (A > PG_AMAX) return false;
    const uint32_t m0 = cd->plan.map_off[r], n_map = cd->plan.map_off[r + 1] - m0;
    const uint16_t* __restrict__ map = cd->plan.map + m0;
    unsigned long long own = 0;
    for (uint32_t a = 0; a < A; ++a) {
        const uint32_t id = c->allele_id[a0 + a];   // (k_crplan_ids has checked id < n_map; no read outside the map either way)
        own |= (unsigned long long)(id < n_map ? map[id] & 0xFFu : 0u) << (8u * a);
    }
    keys->bins = (const pg_combined_bin*)cd->bins + c->geno_off[v];
    keys->A = A;
    keys->own.w = own;
    return true;
}

__global__ __launch_bounds__(PCR_BLOCK) void k_crcalls(const DevContig* __restrict__ contigs, const CRecDesc* __restrict__ desc, uint32_t n_desc,
                                                       const uint64_t* __restrict__ thr_m, const int32_t* __restrict__ thr_e) {
    const uint32_t blk = blockIdx.x;
    const CRecDesc* __restrict__ cd = desc + crec_group_of(desc, n_desc, blk);
    const uint32_t r = (blk - cd->blk0) * PCR_BLOCK + threadIdx.x;
    if (r >= cd->R) return;
    pgc_record_keys keys;
    if (!narrow_keys(contigs + cd->chain, cd, r, &keys)) return;   // k_crcalls_wide's
    unsigned long long rec = pack_no_call(PGX_CALL_DEFERRED);
    if (!keys.any_deferred()) {
        DefinedAllele def;
        def.vcf = cd->plan.vcf_index + cd->plan.vcf_off[r];
        const pgx_record_decision d = pgx_decide_record(keys, (cd->plan.rec_var[r] >> 31) != 0u, def, thr_m, thr_e);
        rec = pack_no_call(d.flags);
        if ((d.flags & 0xFFu) == PGX_CALL_OK) rec = pack_call(def.vcf[d.key >> 16], def.vcf[d.key & 0xFFFFu], d.gq, d.flags);
    }
    ((unsigned long long*)cd->calls)[r] = rec;
}

__global__ __launch_bounds__(PCR_BLOCK) void k_crgl(const DevContig* __restrict__ contigs, const CRecDesc* __restrict__ desc, uint32_t n_desc) {
    const uint32_t blk = blockIdx.x;
    const CRecDesc* __restrict__ cd = desc + crec_group_of(desc, n_desc, blk);
    const uint32_t r = (blk - cd->blk0) * PCR_BLOCK + threadIdx.x;
    if (r >= cd->R) return;
    pgc_record_keys keys;
    if (!narrow_keys(contigs + cd->chain, cd, r, &keys)) return;   // k_crgl_wide's
    GlStore store;
    store.cd = cd;
    store.r = r;
    if (keys.any_deferred()) {
        const uint32_t n_values = (uint32_t)(cd->gl_off[r + 1] - cd->gl_off[r]);
        for (uint32_t i = 0; i < n_values; ++i) store(i, pgx_gl_deferred());
        return;
    }
    VcfIndexOf vcf;
    vcf.vcf = cd->plan.vcf_index;
    vcf.at = cd->plan.vcf_off[r];
    pgx_record_gl(keys, cd->plan.vcf_off[r + 1] - vcf.at, (cd->plan.rec_var[r] >> 31) != 0u, vcf, store);
}

// One lane per record of every group in the list: record r of bubble v holds every allele id of v (the first chain's: the
// members' are known equal, k_combine_check) against the length of its map; the lowest (group << 32 | v) stays in *hit.
__global__ __launch_bounds__(PCR_BLOCK) void k_crplan_ids(const DevContig* __restrict__ contigs, const CRecDesc* __restrict__ desc, uint32_t n_desc,
                                                          unsigned long long* __restrict__ hit) {
    const uint32_t blk = blockIdx.x;
    const CRecDesc* __restrict__ cd = desc + crec_group_of(desc, n_desc, blk);
    const uint32_t r = (blk - cd->blk0) * PCR_BLOCK + threadIdx.x;
    if (r >= cd->R) return;
    const DevContig* __restrict__ c = contigs + cd->chain;
    const uint32_t v = cd->plan.rec_var[r] & 0x7FFFFFFFu;
    const uint32_t a0 = c->allele_off[v], a1 = c->allele_off[v + 1];
    const uint32_t n_map = cd->plan.map_off[r + 1] - cd->plan.map_off[r];
    bool outside = false;
    for (uint32_t a = a0; a < a1; ++a) outside = outside || c->allele_id[a] >= n_map;
    if (outside) atomicMin(hit, ((unsigned long long)cd->group << 32) | v);
}

// ---------------------------------------------------------------------------------------------------------------
//  The wave-per-record kernels.  What both do up to the folded map is wide_fold.
// ---------------------------------------------------------------------------------------------------------------
struct PgxSlot {   // a staged value: 16 bytes
    unsigned long long m;
    int32_t e, pad;
};
__device__ __forceinline__ pgx slot_get(const PgxSlot* s) { pgx r; r.m = s->m; r.e = s->e; return r; }
__device__ __forceinline__ void slot_put(PgxSlot* s, pgx x) { s->m = x.m; s->e = x.e; }

__device__ __forceinline__ pg_combined_bin bin_of_words(uint4 w) {
    pg_combined_bin b;
    b.m = (uint64_t)w.x | ((uint64_t)w.y << 32);
    b.e = (int32_t)w.z;
    b.flags = w.w;
    return b;
}
__device__ __forceinline__ pgx value_of(pg_combined_bin b) {
    pgx x;
    x.m = b.m;
    x.e = b.m ? b.e : 0;
    return x;
}

#define PCR_FOLDED 0u     // F holds the record's folded map, *sum2 the renormalising sum (0 for a record without undefined alleles)
#define PCR_EMPTY 1u      // no key: F[(0,0)] = 1
#define PCR_NONE 2u       // every held value zero
#define PCR_DEFERRED 3u   // a deferred bin, or the largest value below the cut

struct WideRecord {
    const uint16_t* vcf;   // the record's vcf_index
    uint32_t nA, K;        // its alleles, its genotype pairs
    bool undef;
};

// (value, key) of two lanes' bests: the later key of equal values wins, a lane without keys never does
__device__ __forceinline__ bool top2_other_wins(const pgx_top2& mine, pgx o_best, unsigned long long o_key) {
    if (o_key == PGX_NO_KEY) return false;
    if (mine.best_key == PGX_NO_KEY) return true;
    const int c = pgx_cmp(o_best, mine.best);
    return c > 0 || (c == 0 && o_key > mine.best_key);
}

// record r (the same on every lane of the block): s_own, Q and F are the block's; the answer is the same on every lane
__device__ __forceinline__ uint32_t wide_fold(const DevContig* __restrict__ c, const CRecDesc* __restrict__ cd, uint32_t r, uint32_t lane,
                                              uint16_t* s_own, PgxSlot* __restrict__ Q, PgxSlot* __restrict__ F, WideRecord* w, pgx* sum2_out) {
    const uint32_t rv = cd->plan.rec_var[r], v = rv & 0x7FFFFFFFu;
    const uint32_t a0 = c->allele_off[v];
    const uint32_t A = c->allele_off[v + 1] - a0;
    const uint32_t n = A * (A + 1u) / 2u;
    const uint32_t m0 = cd->plan.map_off[r], n_map = cd->plan.map_off[r + 1] - m0;
    const uint16_t* __restrict__ map = cd->plan.map + m0;
    const uint32_t vcf0 = cd->plan.vcf_off[r], nA = cd->plan.vcf_off[r + 1] - vcf0;
    const uint16_t* __restrict__ vcf = cd->plan.vcf_index + vcf0;
    const uint32_t K = nA * (nA + 1u) / 2u;
    const uint4* __restrict__ bins = (const uint4*)cd->bins + c->geno_off[v];
    w->vcf = vcf;
    w->nA = nA;
    w->K = K;
    w->undef = (rv >> 31) != 0u;
    for (uint32_t a = lane; a < A; a += PCR_WBLOCK) {
        const uint32_t id = c->allele_id[a0 + a];   // (k_crplan_ids has checked id < n_map; no read outside the map either way)
        s_own[a] = id < n_map ? map[id] : (uint16_t)0u;
    }
    __syncthreads();
    // the bubble's sum, key after key in the map's order, by every lane alike
    pgx sum = pgx_zero(), largest = pgx_zero();
    uint32_t n_keys = 0;
    bool deferred = false;
    for (uint32_t i = 0; i < n; ++i) {
        const pg_combined_bin b = bin_of_words(bins[i]);
        if (!(b.flags & PG_COMBINED_PRESENT)) continue;
        ++n_keys;
        if (b.flags & PG_COMBINED_DEFERRED) { deferred = true; continue; }
        const pgx x = value_of(b);
        sum = pgx_add(sum, x);
        if (pgx_cmp(x, largest) > 0) largest = x;
    }
    if (deferred) return PCR_DEFERRED;
    if (n_keys == 0) return PCR_EMPTY;
    if (sum.m == 0) return PCR_NONE;
    if (pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) return PCR_DEFERRED;
    // the quotients: lane l takes the bins l, l + 64, ...; a bin that is no key stages 0, which changes no rounded sum
    for (uint32_t i = lane; i < n; i += PCR_WBLOCK) {
        const pg_combined_bin b = bin_of_words(bins[i]);
        slot_put(Q + i, (b.flags & PG_COMBINED_PRESENT) ? pgx_div(value_of(b), sum) : pgx_zero());
    }
    __syncthreads();
    // the fold: key (ra, rb) receives the keys (a, b) whose slots carry ra and rb, in the bubble's order
    for (uint32_t k = lane; k < K; k += PCR_WBLOCK) {
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
    if (w->undef) {
        uint32_t k = 0;
        for (uint32_t ra = 0; ra < nA; ++ra) {
            if (vcf[ra] == 0xFFFFu) { k += nA - ra; continue; }
            for (uint32_t rb = ra; rb < nA; ++rb, ++k)
                if (vcf[rb] != 0xFFFFu) sum2 = pgx_add(sum2, slot_get(F + k));
        }
    }
    *sum2_out = sum2;
    return PCR_FOLDED;
}

__global__ __launch_bounds__(PCR_WBLOCK) void k_crcalls_wide(const DevContig* __restrict__ contigs, const CRecDesc* __restrict__ desc,
                                                             const uint2* __restrict__ list, uint32_t n_list, PgxSlot* __restrict__ stage,
                                                             uint32_t max_bins, uint32_t stride, const uint64_t* __restrict__ thr_m,
                                                             const int32_t* __restrict__ thr_e) {
    __shared__ uint16_t s_own[PG_MAX_ALLELES_PER_VARIANT];   // per slot: its record allele
    const uint32_t lane = threadIdx.x;
    PgxSlot* __restrict__ Q = stage + (size_t)blockIdx.x * stride;   // [max_bins] the bubble's quotients
    PgxSlot* __restrict__ F = Q + max_bins;                          // [stride - max_bins] the folded map
    for (uint32_t entry = blockIdx.x; entry < n_list; entry += gridDim.x) {
        __syncthreads();   // the previous record's s_own, Q and F are done with
        const uint2 e = list[entry];   // {descriptor, record}
        const CRecDesc* __restrict__ cd = desc + e.x;
        const uint32_t r = e.y;
        unsigned long long* __restrict__ out = (unsigned long long*)cd->calls;
        WideRecord w;
        pgx sum2;
        const uint32_t st = wide_fold(contigs + cd->chain, cd, r, lane, s_own, Q, F, &w, &sum2);
        if (st != PCR_FOLDED || (w.undef && sum2.m == 0)) {   // (the same on every lane)
            if (lane == 0)
                out[r] = st == PCR_EMPTY ? pack_call(0u, 0u, PG_GQ_CERTAIN, PGX_CALL_OK | PGX_CALL_EMPTY)
                                         : pack_no_call(st == PCR_DEFERRED ? PGX_CALL_DEFERRED : PGX_CALL_NONE);
            continue;
        }
        // the likeliest genotype and the runner-up
        pgx_top2 t;
        pgx_top2_init(&t);
        for (uint32_t k = lane; k < w.K; k += PCR_WBLOCK) {
            uint32_t ra = 0, rest = k;
            while (rest >= w.nA - ra) { rest -= w.nA - ra; ++ra; }
            const uint32_t rb = ra + rest;
            if (w.undef && (w.vcf[ra] == 0xFFFFu || w.vcf[rb] == 0xFFFFu)) continue;
            pgx f = slot_get(F + k);
            if (w.undef) f = pgx_div(f, sum2);
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
        else rec = pack_call(w.vcf[(uint32_t)(t.best_key >> 16)], w.vcf[(uint32_t)(t.best_key & 0xFFFFu)], pgx_gq_of_best(t.best, thr_m, thr_e), PGX_CALL_OK);
        out[r] = rec;
    }
}

__global__ __launch_bounds__(PCR_WBLOCK) void k_crgl_wide(const DevContig* __restrict__ contigs, const CRecDesc* __restrict__ desc,
                                                          const uint2* __restrict__ list, uint32_t n_list, PgxSlot* __restrict__ stage,
                                                          uint32_t max_bins, uint32_t stride) {
    __shared__ uint16_t s_own[PG_MAX_ALLELES_PER_VARIANT];   // per slot: its record allele
    const uint32_t lane = threadIdx.x;
    PgxSlot* __restrict__ Q = stage + (size_t)blockIdx.x * stride;   // [max_bins] the bubble's quotients
    PgxSlot* __restrict__ F = Q + max_bins;                          // [stride - max_bins] the folded map
    for (uint32_t entry = blockIdx.x; entry < n_list; entry += gridDim.x) {
        __syncthreads();   // the previous record's s_own, Q and F are done with
        const uint2 e = list[entry];   // {descriptor, record}
        const CRecDesc* __restrict__ cd = desc + e.x;
        const uint32_t r = e.y;
        const uint64_t o0 = cd->gl_off[r];
        uint32_t* __restrict__ out = (uint32_t*)cd->gl + o0;
        WideRecord w;
        pgx sum2;
        const uint32_t st = wide_fold(contigs + cd->chain, cd, r, lane, s_own, Q, F, &w, &sum2);
        if (st != PCR_FOLDED) {   // (the same on every lane)
            const uint32_t n_values = (uint32_t)(cd->gl_off[r + 1] - o0);
            const uint32_t g = gl_word(st == PCR_DEFERRED ? pgx_gl_deferred() : pgx_gl_neg_inf());
            for (uint32_t i = lane; i < n_values; i += PCR_WBLOCK) out[i] = (st == PCR_EMPTY && i == 0) ? gl_word(pgx_gl_of(0, 0)) : g;
            continue;
        }
        // the digits: lane l converts and stores the keys l, l + 64, ...
        for (uint32_t k = lane; k < w.K; k += PCR_WBLOCK) {
            uint32_t ra = 0, rest = k;
            while (rest >= w.nA - ra) { rest -= w.nA - ra; ++ra; }
            const uint32_t va = w.vcf[ra], vb = w.vcf[ra + rest];
            if (va == 0xFFFFu || vb == 0xFFFFu) continue;
            pgx f = slot_get(F + k);
            if (sum2.m != 0) f = pgx_div(f, sum2);
            out[vb * (vb + 1u) / 2u + va] = gl_word(pgx_gl(f));
        }
    }
}

}  // namespace

extern "C" void pgk_launch_crcalls(const DevContig* d_contigs, const CRecDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide,
                                   uint32_t n_wide, void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, const uint64_t* d_thr_m,
                                   const int32_t* d_thr_e, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_crcalls, dim3(n_blocks), dim3(PCR_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_thr_m, d_thr_e);
    if (n_wide && n_slots)
        hipLaunchKernelGGL(k_crcalls_wide, dim3(n_slots < n_wide ? n_slots : n_wide), dim3(PCR_WBLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, n_wide,
                           (PgxSlot*)d_stage, max_bins, stride, d_thr_m, d_thr_e);
}

extern "C" void pgk_launch_crgl(const DevContig* d_contigs, const CRecDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                                void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_crgl, dim3(n_blocks), dim3(PCR_BLOCK), 0, s, d_contigs, d_desc, n_desc);
    if (n_wide && n_slots)
        hipLaunchKernelGGL(k_crgl_wide, dim3(n_slots < n_wide ? n_slots : n_wide), dim3(PCR_WBLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, n_wide,
                           (PgxSlot*)d_stage, max_bins, stride);
}

extern "C" void pgk_launch_crplan_ids(const DevContig* d_contigs, const CRecDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, void* d_hit, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_crplan_ids, dim3(n_blocks), dim3(PCR_BLOCK), 0, s, d_contigs, d_desc, n_desc, (unsigned long long*)d_hit);
}

extern "C" uint32_t pgk_combined_records_block(void) { return PCR_BLOCK; }
