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
#include "pg_launch.h"

#define PC_BLOCK 256
#define PC_WAVES (PC_BLOCK / 64)

namespace {

__device__ __forceinline__ unsigned long long pack_call(uint32_t a1, uint32_t a2, uint32_t gq, uint32_t flags) {
    return (unsigned long long)(a1 & 0xFFFFu) | ((unsigned long long)(a2 & 0xFFFFu) << 16) | ((unsigned long long)(gq & 0xFFFFu) << 32) |
           ((unsigned long long)(flags & 0xFFFFu) << 48);
}
__device__ __forceinline__ unsigned long long pack_no_call(uint32_t flags) { return pack_call(0xFFFFu, 0xFFFFu, 0u, flags); }

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

// (value, bin) pairs ordered by value, then by bin: the reference's `>=` keeps the LAST of equal maxima
__device__ __forceinline__ bool wide_better(pgx q, uint32_t bin, pgx best, uint32_t best_bin) {
    const int c = pgx_cmp(q, best);
    return c > 0 || (c == 0 && bin > best_bin);
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

}  // namespace

extern "C" void pgk_launch_calls(const DevContig* d_contigs, const CallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide,
                                 uint32_t n_wide, const uint64_t* d_thr_m, const int32_t* d_thr_e, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_calls, dim3(n_blocks), dim3(PC_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_thr_m, d_thr_e);
    if (n_wide)
        hipLaunchKernelGGL(k_calls_wide, dim3((n_wide + PC_WAVES - 1) / PC_WAVES), dim3(PC_BLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, n_wide,
                           d_thr_m, d_thr_e);
}
extern "C" uint32_t pgk_calls_block(void) { return PC_BLOCK; }
