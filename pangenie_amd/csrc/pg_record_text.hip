// pg_record_text.hip — the bytes of the VCF sample column `GT:GQ:GL:KC` formed on the device (gfx950), DESIGN.md §4e-6.
//
// The rule is pgx_record_put of pg_calls.h, the same functions the host compiles.  The text of all records of a launch is
// PACKED: no gap between records or chains, so where a byte lies follows from the lengths before it — a scan — and from
// nothing else: no atomics anywhere.
//
//   k_rtext_len_wide  one wave per listed wide record: its length, the values spread over the lanes
//   k_rtext_len       one lane per record forms the length (the format into a sink that counts); a block scans its 256
//                     lengths: every record's offset inside the block, and the block's sum
//   k_rtext_sums      one workgroup scans the block sums: every block's first byte (64 bits), the total behind the last
//   k_rtext_emit      a workgroup formats its block of records into an LDS stage, lane per record, then writes the stage to
//                     the block's contiguous byte range with 16-byte stores.  The stage is laid out at the residue mod 16
//                     of the range's first byte, so LDS and global chunks line up; head and tail of the range, which are not
//                     aligned, go out as bytes.  A block whose text is longer than the stage takes it window after window: a
//                     record that crosses the end of a window is formatted once per window through a sink that clips.
//   k_rtext_emit_wide one wave per listed wide record, 64 values a step through a stage of its own
// A record is WIDE if the bound of its text (pgx_record_text_bound(1, n_gl)) is more than a quarter of the stage: one lane
// would format it alone while 255 wait.  The block kernels leave such records' bytes out (windows end and begin at them).
// One launch of each covers every chain of a job: a descriptor per chain, a block finds its chain by bisection.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_calls.h"
#include "pg_launch.h"
#include "pg_text_scan.h"   // wave_incl_scan, block_excl_scan, block_sums_scan, rtext_flush: shared with pg_record_lines.hip

#define RT_BLOCK PGT_BLOCK
#define RT_WAVES PGT_WAVES
#define RT_STAGE 32768u               // bytes of k_rtext_emit's stage: four workgroups share a CU's 160 KB
#define RT_WINDOW (RT_STAGE - 16u)    // bytes of text a window takes at most (the stage begins at the range's residue mod 16)
#define RT_WIDE_BOUND (RT_STAGE / 4u)
#define RTW_BLOCK 64
#define RTW_STAGE 4096u               // bytes of k_rtext_emit_wide's stage
#define RTW_STEP (64u * PGX_TEXT_PER_VALUE)   // the most 64 values and their commas take

namespace {

__device__ __forceinline__ uint32_t rtext_chain_of(const RTextDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool rtext_is_wide(uint32_t n_gl) { return pgx_record_text_bound(1, n_gl) > RT_WIDE_BOUND; }

// what the text of record r of a descriptor is made from
struct RecIn {
    pg_call call;
    const pg_gl* gl;
    uint32_t n_gl, kc;
    bool no_call;
};
__device__ __forceinline__ RecIn rtext_record(const DevContig* __restrict__ contigs, const RTextDesc& d, uint32_t r) {
    RecIn in;
    const unsigned long long w = ((const unsigned long long*)d.calls)[r];
    in.call.allele_1 = (uint16_t)w; in.call.allele_2 = (uint16_t)(w >> 16); in.call.gq = (uint16_t)(w >> 32); in.call.flags = (uint16_t)(w >> 48);
    const uint64_t g0 = d.gl_off[r];
    in.gl = (const pg_gl*)d.gl + g0;
    in.n_gl = (uint32_t)(d.gl_off[r + 1] - g0);
    if (d.rec_var) {   // a job's chain: KC and UK of the record's bubble, both 0 for a chain without a kept column (pg_job_fetch's rule)
        const DevContig* __restrict__ c = contigs + d.chain;
        const uint32_t v = d.rec_var[r] & 0x7FFFFFFFu;
        const bool cols = *c->n_cols != 0;
        in.kc = cols ? c->cov[v] : 0u;
        const uint32_t uk = cols ? c->kmer_off[v + 1] - c->kmer_off[v] : 0u;
        in.no_call = d.ignore_imputed && uk == 0;
    } else {           // the unit entry point: both per record
        in.kc = d.kc[r];
        in.no_call = d.no_call && d.no_call[r] != 0;
    }
    return in;
}

// stores into an LDS stage what falls into [lo, hi) of it
struct ClipSink {
    unsigned char* stage;
    int32_t pos, lo, hi;
    __device__ __forceinline__ void put(char c) {
        if (pos >= lo && pos < hi) stage[pos] = (unsigned char)c;
        ++pos;
    }
};

__global__ __launch_bounds__(RT_BLOCK) void k_rtext_len_wide(const DevContig* __restrict__ contigs, const RTextDesc* __restrict__ desc,
                                                             const uint2* __restrict__ list, uint32_t n_list, uint32_t* __restrict__ wlen,
                                                             uint32_t* __restrict__ loc) {
    const uint32_t entry = blockIdx.x * RT_WAVES + threadIdx.x / 64u, lane = threadIdx.x % 64u;
    if (entry >= n_list) return;   // (whole waves leave)
    const uint2 e = list[entry];   // {descriptor, record}
    const RTextDesc d = desc[e.x];
    const RecIn in = rtext_record(contigs, d, e.y);
    pgx_count_sink s;
    s.n = 0;
    uint32_t refused = 0;
    for (uint32_t i = lane; i < in.n_gl; i += 64u) {
        const pg_gl g = in.gl[i];
        if (pgx_gl_refused(g)) refused = 1;
        else pgx_gl_put(g, s);
    }
    uint32_t n = s.n;
    for (uint32_t o = 32; o; o >>= 1) { n += __shfl_xor(n, o, 64); refused |= __shfl_xor(refused, o, 64); }
    if (lane) return;
    if (refused || (in.call.flags & 0xFFu) == PGX_CALL_DEFERRED || in.n_gl < 3u) n = 0;
    else {
        pgx_count_sink t;
        t.n = 0;
        pgx_record_head_put(in.call, in.no_call, t);
        pgx_record_tail_put(in.kc, t);
        n += t.n + (in.n_gl - 1u);
    }
    wlen[entry] = n;
    loc[d.rec0 + e.y] = n;   // (k_rtext_len reads it here and puts the record's offset in its place)
}

// loc[g]: going in, the length of a wide record g (k_rtext_len_wide's); coming out, the
// first byte of record g inside its block.  bsum[b]: the bytes of block b.
__global__ __launch_bounds__(RT_BLOCK) void k_rtext_len(const DevContig* __restrict__ contigs, const RTextDesc* __restrict__ desc, uint32_t n_desc,
                                                        uint32_t* __restrict__ loc, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t s_wave[RT_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const RTextDesc d = desc[rtext_chain_of(desc, n_desc, blk)];
    const uint32_t r = (blk - d.blk0) * RT_BLOCK + tid;
    uint32_t len = 0;
    if (r < d.R) {
        const RecIn in = rtext_record(contigs, d, r);
        len = rtext_is_wide(in.n_gl) ? loc[d.rec0 + r] : pgx_record_text_len(in.call, in.gl, in.n_gl, in.kc, in.no_call);
    }
    uint32_t total;
    const uint32_t before = block_excl_scan(len, s_wave, &total);
    if (r < d.R) loc[d.rec0 + r] = before;
    if (tid == 0) bsum[blk] = total;
}

// bbase[b] = the bytes of the blocks before b, b = 0 .. n (one workgroup: n is a 256th of the records)
__global__ __launch_bounds__(RT_BLOCK) void k_rtext_sums(const uint32_t* __restrict__ bsum, uint32_t n, unsigned long long* __restrict__ bbase) {
    __shared__ unsigned long long s_wave[RT_WAVES];
    block_sums_scan(bsum, n, bbase, s_wave);
}

__global__ __launch_bounds__(RT_BLOCK) void k_rtext_emit(const DevContig* __restrict__ contigs, const RTextDesc* __restrict__ desc, uint32_t n_desc,
                                                         const uint32_t* __restrict__ loc, const unsigned long long* __restrict__ bbase,
                                                         unsigned long long* __restrict__ off, uint64_t n_records, char* __restrict__ text, uint64_t cap) {
    __shared__ uint4 s_stage[RT_STAGE / 16];
    __shared__ uint32_t s_start[RT_BLOCK + 1];
    __shared__ uint8_t s_wide[RT_BLOCK];
    __shared__ uint32_t s_win[2];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const RTextDesc d = desc[rtext_chain_of(desc, n_desc, blk)];
    const uint32_t r = (blk - d.blk0) * RT_BLOCK + tid;
    const bool valid = r < d.R;
    const uint64_t base = bbase[blk];
    const uint32_t B = (uint32_t)(bbase[blk + 1] - base);   // the block's bytes, wide records' included
    RecIn in;
    in.n_gl = 0;
    uint32_t start = B;
    if (valid) {
        in = rtext_record(contigs, d, r);
        start = loc[d.rec0 + r];
        off[d.rec0 + r] = base + start;
    }
    if (blk == gridDim.x - 1 && tid == 0) off[n_records] = bbase[gridDim.x];
    s_start[tid] = start;
    if (tid == 0) s_start[RT_BLOCK] = B;
    __syncthreads();
    const uint32_t end = s_start[tid + 1], len = end - start;
    const bool wide = valid && len != 0 && rtext_is_wide(in.n_gl);
    s_wide[tid] = wide ? 1 : 0;
    const bool any_wide = __syncthreads_or(wide ? 1 : 0) != 0;
    unsigned char* stage = (unsigned char*)s_stage;
    uint32_t w0 = 0, j = 0;   // (j: thread 0's cursor over the records, used only with wide records in the block)
    for (;;) {
        uint32_t w1;
        if (!any_wide) w1 = B - w0 < RT_WINDOW ? B : w0 + RT_WINDOW;
        else {
            if (tid == 0) {   // the next window: behind the wide records at w0, up to RT_WINDOW bytes, ending at the next wide record
                uint32_t a = w0;
                for (;;) {
                    while (j < RT_BLOCK && s_start[j + 1] <= a) ++j;
                    if (j < RT_BLOCK && s_wide[j]) { a = s_start[j + 1]; ++j; continue; }
                    break;
                }
                uint32_t b = B - a < RT_WINDOW ? B : a + RT_WINDOW;
                for (uint32_t k = j + 1; k < RT_BLOCK && s_start[k] < b; ++k)
                    if (s_wide[k]) { b = s_start[k]; break; }
                s_win[0] = a;
                s_win[1] = a < B ? b : B;
            }
            __syncthreads();
            w0 = s_win[0];
            w1 = s_win[1];
        }
        if (w0 >= B) break;
        const uint64_t g0 = base + w0;
        const uint32_t shift = (uint32_t)(g0 & 15u);
        if (valid && !wide && len != 0 && start < w1 && end > w0) {
            ClipSink s;
            s.stage = stage;
            s.pos = (int32_t)shift + (int32_t)(start - w0);   // (start < w0: the record began in the window before)
            s.lo = (int32_t)shift;
            s.hi = (int32_t)(shift + (w1 - w0));
            pgx_record_put(in.call, in.gl, in.n_gl, in.kc, in.no_call, s);
        }
        __syncthreads();
        rtext_flush<RT_BLOCK>(s_stage, text, g0 - shift, shift, shift + (w1 - w0), cap, tid);
        __syncthreads();
        w0 = w1;
    }
}

__global__ __launch_bounds__(RTW_BLOCK) void k_rtext_emit_wide(const DevContig* __restrict__ contigs, const RTextDesc* __restrict__ desc,
                                                               const uint2* __restrict__ list, const uint32_t* __restrict__ wlen,
                                                               const uint32_t* __restrict__ loc, const unsigned long long* __restrict__ bbase,
                                                               char* __restrict__ text, uint64_t cap) {
    __shared__ uint4 s_stage[RTW_STAGE / 16];
    const uint32_t entry = blockIdx.x, lane = threadIdx.x;
    if (wlen[entry] == 0) return;   // the host's
    const uint2 e = list[entry];    // {descriptor, record}
    const RTextDesc d = desc[e.x];
    const RecIn in = rtext_record(contigs, d, e.y);
    unsigned char* stage = (unsigned char*)s_stage;
    uint64_t gpos = bbase[d.blk0 + e.y / RT_BLOCK] + loc[d.rec0 + e.y];
    uint32_t i0 = 0;
    bool head_done = false, tail_done = false;
    while (!tail_done) {
        const uint32_t shift = (uint32_t)(gpos & 15u);
        uint32_t fill = shift;
        if (!head_done) {   // (every lane forms the head's length; lane 0 stores it)
            ClipSink s;
            s.stage = stage; s.pos = (int32_t)fill; s.lo = lane == 0 ? 0 : (int32_t)RTW_STAGE; s.hi = (int32_t)RTW_STAGE;
            pgx_record_head_put(in.call, in.no_call, s);
            fill = (uint32_t)s.pos;
            head_done = true;
        }
        while (i0 < in.n_gl && fill + RTW_STEP <= RTW_STAGE) {
            const uint32_t i = i0 + lane;
            pg_gl g = pgx_gl_of(0, 0);
            uint32_t mine = 0;
            if (i < in.n_gl) {
                g = in.gl[i];
                pgx_count_sink c;
                c.n = i ? 1u : 0u;
                pgx_gl_put(g, c);
                mine = c.n;
            }
            const uint32_t incl = wave_incl_scan(mine, lane);
            if (i < in.n_gl) {
                ClipSink s;
                s.stage = stage; s.pos = (int32_t)(fill + incl - mine); s.lo = 0; s.hi = (int32_t)RTW_STAGE;
                if (i) s.put(',');
                pgx_gl_put(g, s);
            }
            fill += __shfl(incl, 63, 64);
            i0 += 64u;
        }
        if (i0 >= in.n_gl && fill + PGX_TEXT_PER_RECORD <= RTW_STAGE) {
            ClipSink s;
            s.stage = stage; s.pos = (int32_t)fill; s.lo = lane == 0 ? 0 : (int32_t)RTW_STAGE; s.hi = (int32_t)RTW_STAGE;
            pgx_record_tail_put(in.kc, s);
            fill = (uint32_t)s.pos;
            tail_done = true;
        }
        __syncthreads();
        rtext_flush<RTW_BLOCK>(s_stage, text, gpos - shift, shift, fill, cap, lane);
        __syncthreads();
        gpos += fill - shift;
    }
}

}  // namespace

extern "C" uint32_t pgk_rtext_block(void) { return RT_BLOCK; }
extern "C" uint32_t pgk_rtext_stage_bytes(void) { return RT_STAGE; }
extern "C" uint32_t pgk_rtext_wide_values(void) { return (RT_WIDE_BOUND - PGX_TEXT_PER_RECORD) / PGX_TEXT_PER_VALUE; }

extern "C" void pgk_launch_rtext(const DevContig* d_contigs, const RTextDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                                 uint32_t* d_loc, uint32_t* d_wlen, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off, uint64_t n_records, char* d_text,
                                 uint64_t cap, hipEvent_t emit_begin, hipEvent_t emit_end, hipStream_t s) {
    if (!n_desc || !n_blocks) return;
    if (n_wide)
        hipLaunchKernelGGL(k_rtext_len_wide, dim3((n_wide + RT_WAVES - 1) / RT_WAVES), dim3(RT_BLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, n_wide, d_wlen,
                           d_loc);
    hipLaunchKernelGGL(k_rtext_len, dim3(n_blocks), dim3(RT_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_loc, d_bsum);
    hipLaunchKernelGGL(k_rtext_sums, dim3(1), dim3(RT_BLOCK), 0, s, d_bsum, n_blocks, (unsigned long long*)d_bbase);
    if (emit_begin) (void)hipEventRecord(emit_begin, s);
    hipLaunchKernelGGL(k_rtext_emit, dim3(n_blocks), dim3(RT_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_loc, (const unsigned long long*)d_bbase,
                       (unsigned long long*)d_off, n_records, d_text, cap);
    if (emit_end) (void)hipEventRecord(emit_end, s);
    if (n_wide)
        hipLaunchKernelGGL(k_rtext_emit_wide, dim3(n_wide), dim3(RTW_BLOCK), 0, s, d_contigs, d_desc, (const uint2*)d_wide, d_wlen, d_loc,
                           (const unsigned long long*)d_bbase, d_text, cap);
}
