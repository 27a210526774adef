// pg_record_lines_slot.hip — VCF lines over a SLOTTED prefix joined on the device (gfx950), DESIGN.md §4e-8.
//
// A sampled cohort's chains are index contigs of their own, yet the fixed columns of a chromosome differ between them in
// one number only: UK, the k-mer count of the record's bubble in the chain's reduced panel.  So the prefix is uploaded once
// per chromosome with a slot per record, and the line of record r of an index contig is
//     prefix[r][0 : slot[r]]  dec(UK)  prefix[r][slot[r] :]  ('\t' text_s[r] for every member s in order)  '\n'
// with UK read from the first member's DevContig under pg_job_fetch's rule (as rtext_record of pg_record_text.hip reads it:
// 0 for a chain without a kept column, 16 bits), or from a per-record array (the unit entry point).  A descriptor without
// slots is pg_record_lines.hip's line, byte for byte: one launch carries both kinds of index contig.  Everything else is
// §4e-7's: a line is the host's — length 0 — if any member's text of the record is empty, the lines are packed, a scan
// and nothing else says where a byte lies.
//
//   k_rlslot_len   one lane per line: k_rlines_len's walk over the members' offsets, and the digits of the line's UK
//   k_rlslot_sums  one workgroup scans the block sums (64 bits)
//   k_rlslot_emit  k_rlines_emit's design — one wave per `lpw` lines as one stream of pieces, a wave scan places them, an
//                  LDS stage at the residue mod 16 of the range's first byte, 16-byte stores, windows, big pieces by the
//                  whole wave — with S + 4 pieces a line: head, number, tail, the members' texts, the newline.  The number
//                  has no source: its lane forms each of its at most 5 characters from the value in a register.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_launch.h"
#include "pg_text_scan.h"

#define RLS_BLOCK PGT_BLOCK           // lines a block of k_rlslot_len scans
#define RLS_WAVES PGT_WAVES
#define RLS_EMIT 64                   // threads of k_rlslot_emit: one wave
#define RLS_STAGE 8192u               // bytes of its stage
#define RLS_SMALL 128u                // a piece of at most this many bytes is copied by its lane
#define RLS_MAX_LPW 64u
#define RLS_MAX_PIECES 384u           // pieces of a wave's lines: six steps (64 lines of one or two members)

namespace {

__device__ __forceinline__ uint32_t rlslot_desc_of_len(const RLinesSlotDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].l.blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t rlslot_desc_of_emit(const RLinesSlotDesc* __restrict__ desc, uint32_t n, uint32_t e) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].l.eblk0 <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// UK of record r of a slotted descriptor: the unit entry point's array, or the first member's count under pg_job_fetch's rule
__device__ __forceinline__ uint32_t rlslot_uk(const DevContig* __restrict__ contigs, const RLinesSlotDesc& d, uint32_t r) {
    if (d.uk) return d.uk[r];
    const DevContig* __restrict__ c = contigs + d.chain;
    const uint32_t v = d.rec_var[r] & 0x7FFFFFFFu;
    return *c->n_cols != 0 ? (c->kmer_off[v + 1] - c->kmer_off[v]) & 0xFFFFu : 0u;
}
__device__ __forceinline__ uint32_t rlslot_digits(uint32_t u) { return u < 10u ? 1u : u < 100u ? 2u : u < 1000u ? 3u : u < 10000u ? 4u : 5u; }
// the digits of u as characters, the first in the lowest byte (a register, no local array: that would be scratch)
__device__ __forceinline__ uint64_t rlslot_chars(uint32_t u) {
    uint64_t pk = '0' + u % 10u;
    u /= 10u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (u) {
            pk = (pk << 8) | ('0' + u % 10u);
            u /= 10u;
        }
    return pk;
}

// loc[g]: the first byte of line g inside its block.  bsum[b]: the bytes of block b.
__global__ __launch_bounds__(RLS_BLOCK) void k_rlslot_len(const DevContig* __restrict__ contigs, const RLinesSlotDesc* __restrict__ desc, uint32_t n_desc,
                                                          const RLinesMember* __restrict__ members, uint32_t* __restrict__ loc, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t s_wave[RLS_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const RLinesSlotDesc d = desc[rlslot_desc_of_len(desc, n_desc, blk)];
    const uint32_t r = (blk - d.l.blk0) * RLS_BLOCK + tid;
    uint32_t len = 0;
    if (r < d.l.R) {
        len = (uint32_t)(d.l.prefix_off[r + 1] - d.l.prefix_off[r]) + 1u;   // (the prefix and the newline)
        if (d.slot) len += rlslot_digits(rlslot_uk(contigs, d, r));
        bool host = false;
        for (uint32_t s = 0; s < d.l.S; ++s) {
            const uint64_t* __restrict__ o = members[d.l.mem0 + s].off;
            const uint32_t l = (uint32_t)(o[r + 1] - o[r]);
            host |= l == 0;
            len += l + 1u;                                                   // (a tab in front of it)
        }
        if (host) len = 0;
    }
    uint32_t total;
    const uint32_t before = block_excl_scan(len, s_wave, &total);
    if (r < d.l.R) loc[d.l.line0 + r] = before;
    if (tid == 0) bsum[blk] = total;
}

// bbase[b] = the bytes of the blocks before b, b = 0 .. n
__global__ __launch_bounds__(RLS_BLOCK) void k_rlslot_sums(const uint32_t* __restrict__ bsum, uint32_t n, unsigned long long* __restrict__ bbase) {
    __shared__ unsigned long long s_wave[RLS_WAVES];
    block_sums_scan(bsum, n, bbase, s_wave);
}

__global__ __launch_bounds__(RLS_EMIT) void k_rlslot_emit(const DevContig* __restrict__ contigs, const RLinesSlotDesc* __restrict__ desc, uint32_t n_desc,
                                                          const RLinesMember* __restrict__ members, const uint32_t* __restrict__ loc,
                                                          const unsigned long long* __restrict__ bbase, uint32_t n_blocks, unsigned long long* __restrict__ off,
                                                          uint64_t n_lines, char* __restrict__ out, uint64_t cap) {
    __shared__ uint4 s_stage[RLS_STAGE / 16];
    __shared__ uint32_t s_start[RLS_MAX_LPW + 1];
    const uint32_t e = blockIdx.x, lane = threadIdx.x;
    const RLinesSlotDesc d = desc[rlslot_desc_of_emit(desc, n_desc, e)];
    const uint32_t l0 = (e - d.l.eblk0) * d.l.lpw;                   // the wave's first line (lpw divides RLS_BLOCK: all in one block of the scan)
    const uint32_t n = d.l.R - l0 < d.l.lpw ? d.l.R - l0 : d.l.lpw;
    const uint32_t blk = d.l.blk0 + l0 / RLS_BLOCK;
    const uint64_t base = bbase[blk];
    const uint32_t B = (uint32_t)(bbase[blk + 1] - base);
    for (uint32_t i = lane; i <= n; i += RLS_EMIT) {
        const uint32_t l = l0 + i;
        const bool here = i < n || (l < d.l.R && l % RLS_BLOCK != 0u);   // (the line behind the wave's, if the block has one)
        const uint32_t start = here ? loc[d.l.line0 + l] : B;
        s_start[i] = start;
        if (i < n) off[d.l.line0 + l] = base + start;
    }
    if (e == gridDim.x - 1 && lane == 0) off[n_lines] = bbase[n_blocks];
    __syncthreads();
    const uint32_t first = s_start[0];
    if (s_start[n] == first) return;   // (every line the host's: whole waves leave)
    unsigned char* stage = (unsigned char*)s_stage;
    uint64_t gpos = base + first;
    uint32_t shift = (uint32_t)(gpos & 15u), fill = shift;
    const uint32_t P = d.l.S + 4u, Q = n * P;   // pieces of a line: head, number, tail, the members' texts, the newline
    for (uint32_t q0 = 0; q0 < Q; q0 += RLS_EMIT) {
        const uint32_t q = q0 + lane;
        const char* src = nullptr;
        uint32_t tot = 0, lead = 0;     // lead: the character in front of the piece's bytes, 0 for none
        uint64_t digits = 0;            // the number piece has no source: its characters, the first in the lowest byte
        bool number = false;
        if (q < Q) {
            const uint32_t ll = q / P, p = q - ll * P, r = l0 + ll;
            if (s_start[ll + 1] != s_start[ll]) {
                if (p < 3u) {
                    const uint64_t o = d.l.prefix_off[r];
                    const uint32_t len = (uint32_t)(d.l.prefix_off[r + 1] - o);
                    const uint32_t sl = d.slot ? d.slot[r] : len;   // (no slots: the head is the prefix, number and tail are empty)
                    if (p == 0u) {
                        src = d.l.prefix + o;
                        tot = sl;
                    } else if (p == 2u) {
                        src = d.l.prefix + o + sl;
                        tot = len - sl;
                    } else if (d.slot) {
                        const uint32_t uk = rlslot_uk(contigs, d, r);
                        digits = rlslot_chars(uk);
                        tot = rlslot_digits(uk);
                        number = true;
                    }
                } else if (p < d.l.S + 3u) {
                    const RLinesMember m = members[d.l.mem0 + p - 3u];
                    const uint64_t o = m.off[r];
                    src = m.text + o;
                    lead = '\t';
                    tot = (uint32_t)(m.off[r + 1] - o) + 1u;
                } else {
                    lead = '\n';
                    tot = 1u;
                }
            }
        }
        const uint32_t incl = wave_incl_scan(tot, lane), a = incl - tot;
        const uint32_t T = __shfl(incl, 63, 64);
        const bool big = tot > RLS_SMALL;
        const unsigned long long bigmask = __ballot(big);
        const uint32_t nl = lead ? 1u : 0u;
        uint32_t done = 0;
        while (done < T) {   // the step's T bytes, window by window
            const uint32_t room = RLS_STAGE - fill, w = T - done < room ? T - done : room, w1 = done + w;
            if (!big) {
                const uint32_t x0 = a > done ? a : done, x1 = a + tot < w1 ? a + tot : w1;
                for (uint32_t x = x0; x < x1; ++x) {
                    unsigned char ch;
                    if (number) ch = (unsigned char)(digits >> (8u * (x - a)));
                    else ch = nl && x == a ? (unsigned char)lead : (unsigned char)src[x - a - nl];
                    stage[fill + (x - done)] = ch;
                }
            }
            for (unsigned long long m = bigmask; m; m &= m - 1) {   // (uniform: every lane walks the same mask)
                const int j = __ffsll((long long)m) - 1;
                const uint32_t aj = __shfl(a, j, 64), tj = __shfl(tot, j, 64), leadj = __shfl(lead, j, 64), nj = leadj ? 1u : 0u;
                const uint64_t sj = (uint64_t)__shfl((uint32_t)(uintptr_t)src, j, 64) | ((uint64_t)__shfl((uint32_t)((uintptr_t)src >> 32), j, 64) << 32);
                const char* srcj = (const char*)(uintptr_t)sj;
                const uint32_t y0 = aj > done ? aj : done, y1 = aj + tj < w1 ? aj + tj : w1;
                for (uint32_t x = y0 + lane; x < y1; x += RLS_EMIT) stage[fill + (x - done)] = nj && x == aj ? (unsigned char)leadj : (unsigned char)srcj[x - aj - nj];
            }
            fill += w;
            done = w1;
            if (fill == RLS_STAGE) {
                __syncthreads();
                rtext_flush<RLS_EMIT>(s_stage, out, gpos - shift, shift, fill, cap, lane);
                __syncthreads();
                gpos += fill - shift;   // (a multiple of 16 from here on)
                shift = 0;
                fill = 0;
            }
        }
    }
    __syncthreads();
    if (fill > shift) rtext_flush<RLS_EMIT>(s_stage, out, gpos - shift, shift, fill, cap, lane);
}

}  // namespace

// lines per wave of k_rlslot_emit for S members: the largest power of two with at most RLS_MAX_PIECES pieces, at least 1 and at most 64
extern "C" uint32_t pgk_rlines_slot_lines_per_wave(uint32_t n_members) {
    uint32_t lpw = RLS_MAX_LPW;
    while (lpw > 1u && (uint64_t)lpw * ((uint64_t)n_members + 4u) > RLS_MAX_PIECES) lpw >>= 1;
    return lpw;
}

extern "C" void pgk_launch_rlines_slot(const DevContig* d_contigs, const RLinesSlotDesc* d_desc, uint32_t n_desc, const RLinesMember* d_members,
                                       uint32_t n_blocks, uint32_t n_emit_blocks, uint32_t* d_loc, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off,
                                       uint64_t n_lines, char* d_out, uint64_t cap, hipStream_t s) {
    if (!n_desc || !n_blocks || !n_emit_blocks) return;
    hipLaunchKernelGGL(k_rlslot_len, dim3(n_blocks), dim3(RLS_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_members, d_loc, d_bsum);
    hipLaunchKernelGGL(k_rlslot_sums, dim3(1), dim3(RLS_BLOCK), 0, s, d_bsum, n_blocks, (unsigned long long*)d_bbase);
    hipLaunchKernelGGL(k_rlslot_emit, dim3(n_emit_blocks), dim3(RLS_EMIT), 0, s, d_contigs, d_desc, n_desc, d_members, d_loc,
                       (const unsigned long long*)d_bbase, n_blocks, (unsigned long long*)d_off, n_lines, d_out, cap);
}
