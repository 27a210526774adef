// pg_combine.hip — path subsets put together on the device (gfx950): the chains of one contig over different path
// selections are added up key by key, and the calls are formed from the sums.  DESIGN.md §4e-4.
//
// What the reference's `-a` flow does on the host in long double — GenotypingResult::combine per key over the subsets
// (src/commands.cpp:163-177, src/genotypingresult.cpp:193-198), then normalize, get_likeliest_genotype and
// get_genotype_quality — done where the bins lie, in the integer pairs of pg_calls.h / pg_combine.h.
//
//   k_combine        one lane per BIN of a block's 256 variants (variants with at most PG_AMAX alleles): the S member chains'
//                    12-byte bins are read bin after bin, so a wave's loads of one stream cover contiguous memory; the
//                    bin's variant is found by bisection over the block's bin offsets in LDS; one 16-byte store per bin
//   k_combine_wide   one wave per listed variant with more alleles: lane l takes the bins (a, a + l), (a, a + l + 64), ...
//   k_ccalls         one lane per variant: pgx_decide over the variant's combined bins (pgc_keys)
//   k_ccalls_wide    one wave per listed variant, the structure of k_calls_wide: the sum in bin order by every lane alike,
//                    the divisions and the maximum spread over the lanes, the same tie rule
//   k_combine_check  the layout check of a plan: allele_off and allele_id of a member against the first chain of its group
// One launch of each covers every group of a job: a descriptor per group, a block finds its group by bisection.
// No scratch, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_calls_dev.h"
#include "pg_combine.h"
#include "pg_launch.h"

#define PCB_BLOCK 256
#define PCB_WAVES (PCB_BLOCK / 64)

namespace {

// the last descriptor whose first block is <= b (groups without variants are not in the list)
__device__ __forceinline__ uint32_t combine_group_of(const CombineDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint4 bin_words(pg_combined_bin b) {
    return make_uint4((uint32_t)b.m, (uint32_t)(b.m >> 32), (uint32_t)b.e, b.flags);
}
__device__ __forceinline__ pg_combined_bin bin_of_words(uint4 w) {
    pg_combined_bin b;
    b.m = (uint64_t)w.x | ((uint64_t)w.y << 32);
    b.e = (int32_t)w.z;
    b.flags = w.w;
    return b;
}

// key (slots a <= b, bin g) of variant v folded over the group's chains, in their order
__device__ __forceinline__ pg_combined_bin fold_key(const DevContig* __restrict__ contigs, const uint32_t* __restrict__ mem, uint32_t S, uint32_t v,
                                                    uint32_t sa, uint32_t sb, uint64_t g) {
    pgc_fold f;
    pgc_fold_init(&f);
    for (uint32_t s = 0; s < S; ++s) {
        const DevContig* __restrict__ c = contigs + mem[s];
        if (c->kept[v] && c->allele_present[sa] && c->allele_present[sb]) pgc_fold_take(&f, pgc_summand(c->lik[g], c->lik_exp[g]));
    }
    return pgc_fold_bin(&f);
}

__global__ __launch_bounds__(PCB_BLOCK) void k_combine(const DevContig* __restrict__ contigs, const CombineDesc* __restrict__ desc, uint32_t n_desc,
                                                       const uint32_t* __restrict__ members) {
    __shared__ uint32_t s_goff[PCB_BLOCK + 1];   // first bin of the block's variants, relative to the block's first
    const uint32_t blk = blockIdx.x;
    const CombineDesc cd = desc[combine_group_of(desc, n_desc, blk)];
    const uint32_t v0 = (blk - cd.blk0) * PCB_BLOCK;
    if (v0 >= cd.V) return;
    const uint32_t nv = cd.V - v0 < PCB_BLOCK ? cd.V - v0 : PCB_BLOCK;
    const uint32_t* __restrict__ mem = members + cd.first;
    const DevContig* __restrict__ c0 = contigs + mem[0];
    const uint64_t bin0 = c0->geno_off[v0];
    for (uint32_t i = threadIdx.x; i <= nv; i += PCB_BLOCK) s_goff[i] = (uint32_t)(c0->geno_off[v0 + i] - bin0);
    __syncthreads();
    const uint32_t nb = s_goff[nv];
    uint4* __restrict__ out = (uint4*)cd.bins;
    for (uint32_t r = threadIdx.x; r < nb; r += PCB_BLOCK) {
        uint32_t lo = 0, hi = nv;   // the last variant whose first bin is <= r
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_goff[mid] <= r) lo = mid;
            else hi = mid;
        }
        const uint32_t v = v0 + lo;
        const uint32_t a0 = c0->allele_off[v];
        const uint32_t A = c0->allele_off[v + 1] - a0;
        if (A > PG_AMAX) continue;   // k_combine_wide's
        uint32_t sa, sb;
        pgc_slots_of_bin(A, r - s_goff[lo], &sa, &sb);
        const uint64_t g = bin0 + r;
        out[g] = bin_words(fold_key(contigs, mem, cd.S, v, a0 + sa, a0 + sb, g));
    }
}

__global__ __launch_bounds__(PCB_BLOCK) void k_combine_wide(const DevContig* __restrict__ contigs, const CombineDesc* __restrict__ desc,
                                                            const uint32_t* __restrict__ members, const uint2* __restrict__ list, uint32_t n_list) {
    const uint32_t entry = blockIdx.x * PCB_WAVES + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (entry >= n_list) return;   // (whole waves leave)
    const uint2 e = list[entry];   // {descriptor, variant}
    const CombineDesc cd = desc[e.x];
    const uint32_t v = e.y;
    const uint32_t* __restrict__ mem = members + cd.first;
    const DevContig* __restrict__ c0 = contigs + mem[0];
    const uint32_t a0 = c0->allele_off[v];
    const uint32_t A = c0->allele_off[v + 1] - a0;
    const uint64_t g0 = c0->geno_off[v];
    uint4* __restrict__ out = (uint4*)cd.bins;
    uint32_t row = 0;   // first bin of row a
    for (uint32_t a = 0; a < A; ++a) {
        for (uint32_t b = a + lane; b < A; b += 64u) {
            const uint64_t g = g0 + row + (b - a);
            out[g] = bin_words(fold_key(contigs, mem, cd.S, v, a0 + a, a0 + b, g));
        }
        row += A - a;
    }
}

__global__ __launch_bounds__(PCB_BLOCK) void k_ccalls(const DevContig* __restrict__ contigs, const CombineDesc* __restrict__ desc, uint32_t n_desc,
                                                      const uint32_t* __restrict__ members, const uint64_t* __restrict__ thr_m,
                                                      const int32_t* __restrict__ thr_e) {
    const uint32_t blk = blockIdx.x;
    const CombineDesc cd = desc[combine_group_of(desc, n_desc, blk)];
    const uint32_t v = (blk - cd.blk0) * PCB_BLOCK + threadIdx.x;
    if (v >= cd.V) return;
    const DevContig* __restrict__ c0 = contigs + members[cd.first];
    const uint32_t a0 = c0->allele_off[v];
    const uint32_t A = c0->allele_off[v + 1] - a0;
    if (A > PG_AMAX) return;   // k_ccalls_wide's
    pgc_keys keys;
    keys.bins = (const pg_combined_bin*)cd.bins + c0->geno_off[v];
    keys.n = A * (A + 1u) / 2u;
    keys.i = 0;
    keys.deferred = false;
    const pgx_decision r = pgx_decide(keys, thr_m, thr_e);
    unsigned long long rec = pack_no_call(keys.deferred ? PGX_CALL_DEFERRED : r.flags);
    if (!keys.deferred && r.flags == PGX_CALL_OK) {
        uint32_t sa, sb;
        pgc_slots_of_bin(A, keys.bin_of(r.best), &sa, &sb);
        rec = pack_call(c0->allele_id[a0 + sa], c0->allele_id[a0 + sb], r.gq, PGX_CALL_OK);
    }
    ((unsigned long long*)cd.calls)[v] = rec;
}

__device__ __forceinline__ pgx value_of(pg_combined_bin b) {
    pgx x;
    x.m = b.m;
    x.e = b.m ? b.e : 0;
    return x;
}

__global__ __launch_bounds__(PCB_BLOCK) void k_ccalls_wide(const DevContig* __restrict__ contigs, const CombineDesc* __restrict__ desc,
                                                           const uint32_t* __restrict__ members, const uint2* __restrict__ list, uint32_t n_list,
                                                           const uint64_t* __restrict__ thr_m, const int32_t* __restrict__ thr_e) {
    const uint32_t entry = blockIdx.x * PCB_WAVES + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (entry >= n_list) return;   // (whole waves leave)
    const uint2 e = list[entry];   // {descriptor, variant}
    const CombineDesc cd = desc[e.x];
    const uint32_t v = e.y;
    const DevContig* __restrict__ c0 = contigs + members[cd.first];
    unsigned long long* __restrict__ out = (unsigned long long*)cd.calls;
    const uint32_t a0 = c0->allele_off[v];
    const uint32_t A = c0->allele_off[v + 1] - a0;
    const uint32_t n = A * (A + 1u) / 2u;
    const uint4* __restrict__ bins = (const uint4*)cd.bins + c0->geno_off[v];
    // the sum, key after key in the map's order, by every lane alike
    pgx sum = pgx_zero(), largest = pgx_zero();
    bool deferred = false;
    for (uint32_t i = 0; i < n; ++i) {
        const pg_combined_bin b = bin_of_words(bins[i]);
        if (!(b.flags & PG_COMBINED_PRESENT)) continue;
        if (b.flags & PG_COMBINED_DEFERRED) { deferred = true; continue; }
        const pgx x = value_of(b);
        sum = pgx_add(sum, x);
        if (pgx_cmp(x, largest) > 0) largest = x;
    }
    if (deferred || sum.m == 0 || pgx_below_pow2(largest, PG_CALLS_DEFER_EXP)) {
        if (lane == 0) out[v] = pack_no_call(deferred ? PGX_CALL_DEFERRED : (sum.m == 0 ? PGX_CALL_NONE : PGX_CALL_DEFERRED));
        return;
    }
    // the likeliest genotype: lane l takes the bins l, l + 64, ...
    pgx best = pgx_zero();
    uint32_t best_bin = 0;
    for (uint32_t i = lane; i < n; i += 64u) {
        const pg_combined_bin b = bin_of_words(bins[i]);
        if (!(b.flags & PG_COMBINED_PRESENT)) continue;
        const pgx q = pgx_div(value_of(b), sum);
        if (wide_better(q, i, best, best_bin)) { best = q; best_bin = i; }
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
    for (uint32_t i = lane; i < n; i += 64u) {
        const pg_combined_bin b = bin_of_words(bins[i]);
        if (!(b.flags & PG_COMBINED_PRESENT) || i == best_bin) continue;
        if (pgx_within_tie(best, pgx_div(value_of(b), sum))) tie = true;
    }
    const bool any_tie = __ballot(tie ? 1 : 0) != 0ull;
    if (lane != 0) return;
    if (any_tie) { out[v] = pack_no_call(PGX_CALL_NOT_UNIQUE); return; }
    uint32_t sa, sb;
    pgc_slots_of_bin(A, best_bin, &sa, &sb);
    out[v] = pack_call(c0->allele_id[a0 + sa], c0->allele_id[a0 + sb], pgx_gq_of_best(best, thr_m, thr_e), PGX_CALL_OK);
}

// Every lane that finds a difference stores the same kind of word (1 + its pair): whichever store lands last names a pair that differs.
__global__ __launch_bounds__(PCB_BLOCK) void k_combine_check(const DevContig* __restrict__ contigs, const CombinePair* __restrict__ pairs, uint32_t pair0,
                                                             uint32_t* __restrict__ hit) {
    const uint32_t pair = pair0 + blockIdx.y, i = blockIdx.x * PCB_BLOCK + threadIdx.x;
    const CombinePair p = pairs[pair];
    const DevContig* __restrict__ a = contigs + p.ref;
    const DevContig* __restrict__ b = contigs + p.member;
    bool differ = false;
    if (i <= p.V) differ = a->allele_off[i] != b->allele_off[i];
    if (i < p.sumA) differ = differ || a->allele_id[i] != b->allele_id[i];
    if (differ) *hit = pair + 1u;
}

}  // namespace

extern "C" void pgk_launch_combine(const DevContig* d_contigs, const CombineDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const uint32_t* d_members,
                                   const void* d_wide, uint32_t n_wide, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_combine, dim3(n_blocks), dim3(PCB_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_members);
    if (n_wide)
        hipLaunchKernelGGL(k_combine_wide, dim3((n_wide + PCB_WAVES - 1) / PCB_WAVES), dim3(PCB_BLOCK), 0, s, d_contigs, d_desc, d_members, (const uint2*)d_wide, n_wide);
}

extern "C" void pgk_launch_ccalls(const DevContig* d_contigs, const CombineDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const uint32_t* d_members,
                                  const void* d_wide, uint32_t n_wide, const uint64_t* d_thr_m, const int32_t* d_thr_e, hipStream_t s) {
    if (n_desc && n_blocks) hipLaunchKernelGGL(k_ccalls, dim3(n_blocks), dim3(PCB_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_members, d_thr_m, d_thr_e);
    if (n_wide)
        hipLaunchKernelGGL(k_ccalls_wide, dim3((n_wide + PCB_WAVES - 1) / PCB_WAVES), dim3(PCB_BLOCK), 0, s, d_contigs, d_desc, d_members, (const uint2*)d_wide, n_wide,
                           d_thr_m, d_thr_e);
}

extern "C" void pgk_launch_combine_check(const DevContig* d_contigs, const CombinePair* d_pairs, uint32_t n_pairs, uint32_t max_items, uint32_t* d_hit, hipStream_t s) {
    if (!n_pairs || !max_items) return;
    const uint32_t bx = (max_items + PCB_BLOCK - 1) / PCB_BLOCK;
    for (uint32_t p0 = 0; p0 < n_pairs; p0 += 65535u) {
        const uint32_t np = n_pairs - p0 < 65535u ? n_pairs - p0 : 65535u;
        hipLaunchKernelGGL(k_combine_check, dim3(bx, np), dim3(PCB_BLOCK), 0, s, d_contigs, d_pairs, p0, d_hit);
    }
}

extern "C" uint32_t pgk_combine_block(void) { return PCB_BLOCK; }
