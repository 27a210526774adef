// pg_panel_text.hip — the sample columns of the sampled-panel VCF formed on the device (gfx950), DESIGN.md §4e-10.
//
// The rule is pg_panel.h's, the same functions the host compiles.  From the reduced panel a chain holds on the device
// (path_allele [V x P]) and the record plan of its index contig the packed text of all records of a launch: per record the
// P cells joined by tabs, no gap between records or chains, so where a byte lies follows from the lengths before it — a
// scan — and from nothing else: no atomics anywhere.
//
// A record's text grows with P (up to 255 bytes at 64 paths), so the unit that is scanned is the CELL (r, p), 1 to 4 bytes
// with its tab: a block takes 256 consecutive cells of a chain, adjacent lanes read adjacent path_allele entries, and a
// block's text is at most 1 024 bytes whatever P is: one stage takes it, there are no windows and no wide records.
//
//   k_ptpanel_len   one lane per cell forms the length (the format into a sink that counts); a block scans its 256 lengths
//                   for the block's sum.  The lane of a record's first cell also stores the record's UK — the panel's own
//                   count kmer_off[v + 1] - kmer_off[v] — for the line joiner (RLinesDesc::uk)
//   k_ptpanel_sums  one workgroup scans the block sums: every block's first byte (64 bits), the total behind the last
//   k_ptpanel_emit  a workgroup forms its cells again and scans them (cheaper than an array of 32 bits per cell written and
//                   read back), formats them into an LDS stage, lane per cell, then writes the stage to the block's
//                   contiguous byte range with 16-byte stores.  The stage is laid out at the residue mod 16 of the range's
//                   first byte, so LDS and global chunks line up; head and tail of the range go out as bytes.  The lane of
//                   a record's first cell stores the record's offset.
// One launch of each covers every chain of a job: a descriptor per chain, a block finds its chain by bisection.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_launch.h"
#include "pg_panel.h"
#include "pg_text_scan.h"   // block_excl_scan, block_sums_scan, rtext_flush: shared with the record text, the lines and the phased text

#define PP_BLOCK PGT_BLOCK
#define PP_WAVES PGT_WAVES
#define PP_CELL_BYTES 4u                                  // a tab and `255`
#define PP_STAGE (PP_BLOCK * PP_CELL_BYTES + 16u)         // a block's text and the residue in front of it

namespace {

__device__ __forceinline__ uint32_t ptpanel_chain_of(const PanelDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the cell a lane owns: record r, path p of its descriptor; live = there is such a cell
struct PanelCell {
    uint32_t r, p, v;
    uint16_t x;
    bool live, in_map;
};
__device__ __forceinline__ PanelCell ptpanel_cell(const PanelDesc& d, uint32_t blk, uint32_t tid) {
    PanelCell c;
    const uint64_t q0 = (uint64_t)(blk - d.blk0) * PP_BLOCK;   // the block's first cell; P <= 64: the lanes' cells lie within 5 records of it
    uint64_t r0;
    uint32_t p0;
    if ((q0 >> 32) == 0) { r0 = (uint32_t)q0 / d.P; p0 = (uint32_t)q0 % d.P; }
    else { r0 = q0 / d.P; p0 = (uint32_t)(q0 - r0 * d.P); }
    const uint32_t t = p0 + tid;
    const uint64_t r = r0 + t / d.P;
    c.p = t % d.P;
    c.live = r < d.R;
    c.r = (uint32_t)r; c.v = 0;
    c.x = (uint16_t)PGX_PANEL_UNDEFINED;
    c.in_map = true;
    if (c.live) {
        c.v = d.plan.rec_var[c.r] & 0x7FFFFFFFu;
        const uint32_t m0 = d.plan.map_off[c.r], m1 = d.plan.map_off[c.r + 1], v0 = d.plan.vcf_off[c.r], v1 = d.plan.vcf_off[c.r + 1];
        const uint32_t H = d.path_allele[(size_t)c.v * d.P + c.p];
        // (k_rplan_ids has passed the ids of the allele lists; a panel that was never run may still carry a path allele outside
        // them: nothing is read outside the plan's arrays for it)
        c.in_map = H < m1 - m0 && d.plan.map[m0 + H] < v1 - v0;
        if (c.in_map) c.x = pgx_panel_index(d.plan.map, m0, d.plan.vcf_index, v0, H);
    }
    return c;
}

// stores into an LDS stage; nothing at or behind its end
struct StageSink {
    unsigned char* stage;
    uint32_t pos;
    __device__ __forceinline__ void put(char c) {
        if (pos < PP_STAGE) stage[pos] = (unsigned char)c;
        ++pos;
    }
};

// bsum[b]: the bytes of block b.  *bad = 1 if a path's allele id lies outside a record's map.
__global__ __launch_bounds__(PP_BLOCK) void k_ptpanel_len(const PanelDesc* __restrict__ desc, uint32_t n_desc, uint32_t* __restrict__ bsum, uint32_t* __restrict__ bad) {
    __shared__ uint32_t s_wave[PP_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const PanelDesc d = desc[ptpanel_chain_of(desc, n_desc, blk)];
    const PanelCell c = ptpanel_cell(d, blk, tid);
    uint32_t len = 0;
    if (c.live) {
        len = pgx_panel_cell_len(c.x, c.p == 0);
        if (!c.in_map) *bad = 1u;   // (every lane that finds one stores the same word)
        if (c.p == 0 && d.kmer_off) d.uk[c.r] = pgx_panel_uk(d.kmer_off, c.v);
    }
    uint32_t total;
    (void)block_excl_scan(len, s_wave, &total);
    if (tid == 0) bsum[blk] = total;
}

// bbase[b] = the bytes of the blocks before b, b = 0 .. n (one workgroup: n is a 256th of the cells)
__global__ __launch_bounds__(PP_BLOCK) void k_ptpanel_sums(const uint32_t* __restrict__ bsum, uint32_t n, unsigned long long* __restrict__ bbase) {
    __shared__ unsigned long long s_wave[PP_WAVES];
    block_sums_scan(bsum, n, bbase, s_wave);
}

__global__ __launch_bounds__(PP_BLOCK) void k_ptpanel_emit(const PanelDesc* __restrict__ desc, uint32_t n_desc, const unsigned long long* __restrict__ bbase,
                                                           unsigned long long* __restrict__ off, uint64_t n_records, char* __restrict__ text, uint64_t cap) {
    __shared__ uint4 s_stage[PP_STAGE / 16];
    __shared__ uint32_t s_wave[PP_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const PanelDesc d = desc[ptpanel_chain_of(desc, n_desc, blk)];
    const PanelCell c = ptpanel_cell(d, blk, tid);
    const uint32_t len = c.live ? pgx_panel_cell_len(c.x, c.p == 0) : 0u;
    uint32_t B;   // the block's bytes: at most PP_BLOCK cells of 4
    const uint32_t start = block_excl_scan(len, s_wave, &B);
    const uint64_t base = bbase[blk];
    const uint32_t shift = (uint32_t)(base & 15u);
    if (c.live) {
        if (c.p == 0) off[d.rec0 + c.r] = base + start;
        StageSink s;
        s.stage = (unsigned char*)s_stage;
        s.pos = shift + start;
        pgx_panel_cell_put(c.x, c.p == 0, s);
    }
    if (blk == gridDim.x - 1 && tid == 0) off[n_records] = bbase[gridDim.x];
    __syncthreads();
    const uint32_t end = shift + B < PP_STAGE ? shift + B : PP_STAGE;   // (nothing is read behind the stage)
    rtext_flush<PP_BLOCK>(s_stage, text, base - shift, shift, end, cap, tid);
}

}  // namespace

static_assert(PP_STAGE % 16u == 0, "the stage is whole 16-byte chunks");

extern "C" uint32_t pgk_ptpanel_block(void) { return PP_BLOCK; }
extern "C" uint32_t pgk_ptpanel_stage_bytes(void) { return PP_STAGE; }

extern "C" void pgk_launch_ptpanel(const PanelDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off,
                                   uint64_t n_records, char* d_text, uint64_t cap, uint32_t* d_bad, hipStream_t s) {
    if (!n_desc || !n_blocks) return;
    hipLaunchKernelGGL(k_ptpanel_len, dim3(n_blocks), dim3(PP_BLOCK), 0, s, d_desc, n_desc, d_bsum, d_bad);
    hipLaunchKernelGGL(k_ptpanel_sums, dim3(1), dim3(PP_BLOCK), 0, s, d_bsum, n_blocks, (unsigned long long*)d_bbase);
    hipLaunchKernelGGL(k_ptpanel_emit, dim3(n_blocks), dim3(PP_BLOCK), 0, s, d_desc, n_desc, (const unsigned long long*)d_bbase, (unsigned long long*)d_off,
                       n_records, d_text, cap);
}
