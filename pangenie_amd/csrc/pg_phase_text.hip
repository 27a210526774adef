// pg_phase_text.hip — the phasing column `GT:KC` of a `-p` run formed on the device (gfx950), DESIGN.md §4e-9.
//
// The rule is pg_phase.h's, the same functions the host compiles.  From the Viterbi haplotypes a chain's run leaves on the
// device (pg_viterbi.hip: hap1 / hap2 per variant) first two numbers per VCF record, then the packed text of all records of
// a launch: no gap between records or chains, so where a byte lies follows from the lengths before it — a scan — and from
// nothing else: no atomics anywhere.
//
//   k_rphase      one lane per record: the haplotypes' bubble alleles through the record's map and vcf_index, one 4-byte store
//   k_ptext_len   one lane per record forms the length (the format into a sink that counts); a block scans its 256 lengths:
//                 every record's offset inside the block, and the block's sum
//   k_ptext_sums  one workgroup scans the block sums: every block's first byte (64 bits), the total behind the last
//   k_ptext_emit  a workgroup formats its block of records into an LDS stage, lane per record, then writes the stage to the
//                 block's contiguous byte range with 16-byte stores.  The stage is laid out at the residue mod 16 of the
//                 range's first byte, so LDS and global chunks line up; head and tail of the range go out as bytes.
// A record is at most 13 bytes, a block's text at most 3 328: one stage takes it, there are no windows and no wide records.
// One launch of each covers every chain of a job: a descriptor per chain, a block finds its chain by bisection.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_launch.h"
#include "pg_phase.h"
#include "pg_text_scan.h"   // wave_incl_scan, block_excl_scan, block_sums_scan, rtext_flush: shared with the record text and lines

#define PT_BLOCK PGT_BLOCK
#define PT_WAVES PGT_WAVES
#define PT_STAGE (PT_BLOCK * PGX_PHASE_TEXT_PER_RECORD + 16u)   // a block's text and the residue in front of it

namespace {

template <class Desc>
__device__ __forceinline__ uint32_t ptext_chain_of(const Desc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PT_BLOCK) void k_rphase(const DevContig* __restrict__ contigs, const RPhaseDesc* __restrict__ desc, uint32_t n_desc) {
    const uint32_t blk = blockIdx.x;
    const RPhaseDesc d = desc[ptext_chain_of(desc, n_desc, blk)];
    const uint32_t r = (blk - d.blk0) * PT_BLOCK + threadIdx.x;
    if (r >= d.R) return;
    const uint32_t rv = d.plan.rec_var[r], v = rv & 0x7FFFFFFFu;
    const bool some_undefined = (rv >> 31) != 0;
    uint32_t h1, h2;
    bool keyed;
    if (d.hap1) {   // the unit entry point: all three per variant
        h1 = d.hap1[v]; h2 = d.hap2[v];
        keyed = d.keyed[v] != 0;
    } else {        // a job's chain: what its Viterbi left, and whether the bubble's result holds likelihoods
        const DevContig* __restrict__ c = contigs + d.chain;
        h1 = c->hap1[v]; h2 = c->hap2[v];
        keyed = d.run_genotyping && c->kept[v] != 0;
    }
    const uint32_t m0 = d.plan.map_off[r], v0 = d.plan.vcf_off[r];
    const uint16_t x1 = d.plan.vcf_index[v0 + d.plan.map[m0 + h1]], x2 = d.plan.vcf_index[v0 + d.plan.map[m0 + h2]];
    const pg_phase p = pgx_record_phase(x1, x2, some_undefined, keyed);
    ((uint32_t*)d.out)[r] = (uint32_t)p.allele_1 | ((uint32_t)p.allele_2 << 16);
}

// what the text of record r of a descriptor is made from
struct PhaseIn {
    pg_phase phase;
    uint32_t kc;
    bool no_call;
};
__device__ __forceinline__ PhaseIn ptext_record(const DevContig* __restrict__ contigs, const PTextDesc& d, uint32_t r) {
    PhaseIn in;
    const uint32_t w = ((const uint32_t*)d.phase)[r];
    in.phase.allele_1 = (uint16_t)w; in.phase.allele_2 = (uint16_t)(w >> 16);
    if (d.rec_var) {   // a job's chain: KC and UK of the record's bubble under pg_job_fetch's rule
        const DevContig* __restrict__ c = contigs + d.chain;
        const uint32_t v = d.rec_var[r] & 0x7FFFFFFFu, n_cols = *c->n_cols;
        const bool set = (d.run_genotyping && n_cols != 0) || v < n_cols;   // (the Viterbi sets both at the COLUMN index)
        in.kc = set ? c->cov[v] : 0u;
        const uint32_t uk = set ? c->kmer_off[v + 1] - c->kmer_off[v] : 0u;
        in.no_call = d.ignore_imputed && uk == 0;
    } else {           // the unit entry point: both per record
        in.kc = d.kc[r];
        in.no_call = d.no_call && d.no_call[r] != 0;
    }
    return in;
}

// stores into an LDS stage; nothing at or behind its end
struct StageSink {
    unsigned char* stage;
    uint32_t pos;
    __device__ __forceinline__ void put(char c) {
        if (pos < PT_STAGE) stage[pos] = (unsigned char)c;
        ++pos;
    }
};

// loc[g]: the first byte of record g inside its block.  bsum[b]: the bytes of block b.
__global__ __launch_bounds__(PT_BLOCK) void k_ptext_len(const DevContig* __restrict__ contigs, const PTextDesc* __restrict__ desc, uint32_t n_desc,
                                                        uint32_t* __restrict__ loc, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t s_wave[PT_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const PTextDesc d = desc[ptext_chain_of(desc, n_desc, blk)];
    const uint32_t r = (blk - d.blk0) * PT_BLOCK + tid;
    uint32_t len = 0;
    if (r < d.R) {
        const PhaseIn in = ptext_record(contigs, d, r);
        len = pgx_phase_text_len(in.phase, in.kc, in.no_call);
    }
    uint32_t total;
    const uint32_t before = block_excl_scan(len, s_wave, &total);
    if (r < d.R) loc[d.rec0 + r] = before;
    if (tid == 0) bsum[blk] = total;
}

// bbase[b] = the bytes of the blocks before b, b = 0 .. n (one workgroup: n is a 256th of the records)
__global__ __launch_bounds__(PT_BLOCK) void k_ptext_sums(const uint32_t* __restrict__ bsum, uint32_t n, unsigned long long* __restrict__ bbase) {
    __shared__ unsigned long long s_wave[PT_WAVES];
    block_sums_scan(bsum, n, bbase, s_wave);
}

__global__ __launch_bounds__(PT_BLOCK) void k_ptext_emit(const DevContig* __restrict__ contigs, const PTextDesc* __restrict__ desc, uint32_t n_desc,
                                                         const uint32_t* __restrict__ loc, const unsigned long long* __restrict__ bbase,
                                                         unsigned long long* __restrict__ off, uint64_t n_records, char* __restrict__ text, uint64_t cap) {
    __shared__ uint4 s_stage[PT_STAGE / 16];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const PTextDesc d = desc[ptext_chain_of(desc, n_desc, blk)];
    const uint32_t r = (blk - d.blk0) * PT_BLOCK + tid;
    const uint64_t base = bbase[blk];
    const uint32_t B = (uint32_t)(bbase[blk + 1] - base);   // the block's bytes: at most PT_BLOCK records of 13
    const uint32_t shift = (uint32_t)(base & 15u);
    if (r < d.R) {
        const PhaseIn in = ptext_record(contigs, d, r);
        const uint32_t start = loc[d.rec0 + r];
        off[d.rec0 + r] = base + start;
        StageSink s;
        s.stage = (unsigned char*)s_stage;
        s.pos = shift + start;
        pgx_phase_put(in.phase, in.kc, in.no_call, s);
    }
    if (blk == gridDim.x - 1 && tid == 0) off[n_records] = bbase[gridDim.x];
    __syncthreads();
    const uint32_t end = shift + B < PT_STAGE ? shift + B : PT_STAGE;   // (nothing is read behind the stage)
    rtext_flush<PT_BLOCK>(s_stage, text, base - shift, shift, end, cap, tid);
}

}  // namespace

static_assert(PT_STAGE % 16u == 0, "the stage is whole 16-byte chunks");

extern "C" uint32_t pgk_ptext_block(void) { return PT_BLOCK; }
extern "C" uint32_t pgk_ptext_stage_bytes(void) { return PT_STAGE; }

extern "C" void pgk_launch_rphase(const DevContig* d_contigs, const RPhaseDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, hipStream_t s) {
    if (!n_desc || !n_blocks) return;
    hipLaunchKernelGGL(k_rphase, dim3(n_blocks), dim3(PT_BLOCK), 0, s, d_contigs, d_desc, n_desc);
}

extern "C" void pgk_launch_ptext(const DevContig* d_contigs, const PTextDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, uint32_t* d_loc, uint32_t* d_bsum,
                                 uint64_t* d_bbase, uint64_t* d_off, uint64_t n_records, char* d_text, uint64_t cap, hipStream_t s) {
    if (!n_desc || !n_blocks) return;
    hipLaunchKernelGGL(k_ptext_len, dim3(n_blocks), dim3(PT_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_loc, d_bsum);
    hipLaunchKernelGGL(k_ptext_sums, dim3(1), dim3(PT_BLOCK), 0, s, d_bsum, n_blocks, (unsigned long long*)d_bbase);
    hipLaunchKernelGGL(k_ptext_emit, dim3(n_blocks), dim3(PT_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_loc, (const unsigned long long*)d_bbase,
                       (unsigned long long*)d_off, n_records, d_text, cap);
}
