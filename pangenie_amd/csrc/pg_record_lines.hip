// pg_record_lines.hip — whole VCF lines of a cohort joined on the device (gfx950), DESIGN.md §4e-7 and §4e-8.
//
// The line of record r of an index contig is  prefix[r] ('\t' text_s[r] for every member s in order) '\n':  the caller's fixed
// columns, then every member's bytes of that record (pg_record_text.hip's, or any bytes: they are opaque here).  A line is
// the host's — length 0 — if any member's text of the record is empty.  The lines of a launch are PACKED, so where a byte
// lies follows from the lengths before it — a scan — and from nothing else: no atomics anywhere.
//
// A SLOTTED prefix (§4e-8): a sampled cohort's chains are index contigs of their own, yet the fixed columns of a chromosome
// differ between them in one number only: UK, the k-mer count of the record's bubble in the chain's reduced panel.  So the
// prefix is uploaded once per chromosome with a slot per record, and the line begins
//     prefix[r][0 : slot[r]]  dec(UK)  prefix[r][slot[r] :]
// with UK read from the first member's DevContig under pg_job_fetch's rule (as rtext_record of pg_record_text.hip reads it:
// 0 for a chain without a kept column, 16 bits), or from a per-record array (the unit entry point).
//
// k_rlines_len and k_rlines_emit are templates on SLOT.  SLOT = false: no descriptor's slot fields are read, a line has
// S + 2 pieces, and the kernels hold none of the number's code.  SLOT = true: S + 4 pieces; a descriptor without slots gives
// the plain line, byte for byte, so one launch carries both kinds of index contig.
//
//   k_rlines_len   one lane per line walks the members' offsets (adjacent lanes read adjacent offsets of one member) and, SLOT,
//                  counts the digits of the line's UK; a block scans its 256 lengths: every line's offset inside the block,
//                  and the block's sum
//   k_rlines_sums  one workgroup scans the block sums: every block's first byte (64 bits), the total behind the last
//   k_rlines_emit  one wave takes `lpw` consecutive lines — a power of two, 64 for one member down to 1 for many — as ONE
//                  stream of pieces: per line the prefix (SLOT: its head, the number, its tail), S times a tab and a text,
//                  the newline.  64 pieces a step: a wave scan of their lengths gives each its place, the lanes copy their
//                  pieces into an LDS stage, and the stage goes to its contiguous byte range with 16-byte stores whenever
//                  it is full.  The stage is laid out at the residue mod 16 of the range's first byte, so LDS and global
//                  chunks line up; head and tail go out as bytes.  A step longer than the stage's room is taken window by
//                  window: a lane copies what of its piece falls into the window.  A piece of more than RL_SMALL bytes — an
//                  ALT column of a structural variant — is copied by the whole wave, 64 bytes abreast, instead of by its
//                  lane alone.  The number has no source: its lane forms each of its at most 5 characters from the value
//                  in a register.
// Since consecutive lines are adjacent in the output, the S = 1 case needs no kernel of its own: 64 lines of about 100
// bytes are one stream of 192 pieces.  One launch of each kernel covers every index contig: a descriptor per contig, a
// block finds its own by bisection.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_launch.h"
#include "pg_text_scan.h"

#define RL_BLOCK PGT_BLOCK            // lines a block of k_rlines_len scans
#define RL_WAVES PGT_WAVES
#define RL_EMIT 64                    // threads of k_rlines_emit: one wave
#define RL_STAGE 8192u                // bytes of its stage: far more than two workgroups share a CU's 160 KB
#define RL_SMALL 128u                 // a piece of at most this many bytes is copied by its lane
#define RL_MAX_LPW 64u
#define RL_MAX_PIECES 256u            // pieces of a wave's lines: four steps
#define RL_MAX_PIECES_SLOT 384u       // ... over slotted prefixes: six steps (64 lines of one or two members)

namespace {

__device__ __forceinline__ uint32_t rlines_desc_of_len(const RLinesDesc* __restrict__ desc, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].blk0 <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t rlines_desc_of_emit(const RLinesDesc* __restrict__ desc, uint32_t n, uint32_t e) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (desc[mid].eblk0 <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// UK of record r of a slotted descriptor: the unit entry point's array, or the first member's count under pg_job_fetch's rule
__device__ __forceinline__ uint32_t rlines_uk(const DevContig* __restrict__ contigs, const RLinesDesc& d, uint32_t r) {
    if (d.uk) return d.uk[r];
    const DevContig* __restrict__ c = contigs + d.chain;
    const uint32_t v = d.rec_var[r] & 0x7FFFFFFFu;
    return *c->n_cols != 0 ? (c->kmer_off[v + 1] - c->kmer_off[v]) & 0xFFFFu : 0u;
}
__device__ __forceinline__ uint32_t rlines_digits(uint32_t u) { return u < 10u ? 1u : u < 100u ? 2u : u < 1000u ? 3u : u < 10000u ? 4u : 5u; }
// the digits of u as characters, the first in the lowest byte (a register, no local array: that would be scratch)
__device__ __forceinline__ uint64_t rlines_chars(uint32_t u) {
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
template <bool SLOT>
__global__ __launch_bounds__(RL_BLOCK) void k_rlines_len(const DevContig* __restrict__ contigs, const RLinesDesc* __restrict__ desc, uint32_t n_desc,
                                                         const RLinesMember* __restrict__ members, uint32_t* __restrict__ loc, uint32_t* __restrict__ bsum) {
    __shared__ uint32_t s_wave[RL_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const RLinesDesc d = desc[rlines_desc_of_len(desc, n_desc, blk)];
    const uint32_t r = (blk - d.blk0) * RL_BLOCK + tid;
    uint32_t len = 0;
    if (r < d.R) {
        len = (uint32_t)(d.prefix_off[r + 1] - d.prefix_off[r]) + 1u;   // (the prefix and the newline)
        if constexpr (SLOT)
            if (d.slot) len += rlines_digits(rlines_uk(contigs, d, r));
        bool host = false;
        for (uint32_t s = 0; s < d.S; ++s) {
            const uint64_t* __restrict__ o = members[d.mem0 + s].off;
            const uint32_t l = (uint32_t)(o[r + 1] - o[r]);
            host |= l == 0;
            len += l + 1u;                                               // (a tab in front of it)
        }
        if (host) len = 0;
    }
    uint32_t total;
    const uint32_t before = block_excl_scan(len, s_wave, &total);
    if (r < d.R) loc[d.line0 + r] = before;
    if (tid == 0) bsum[blk] = total;
}

// bbase[b] = the bytes of the blocks before b, b = 0 .. n
__global__ __launch_bounds__(RL_BLOCK) void k_rlines_sums(const uint32_t* __restrict__ bsum, uint32_t n, unsigned long long* __restrict__ bbase) {
    __shared__ unsigned long long s_wave[RL_WAVES];
    block_sums_scan(bsum, n, bbase, s_wave);
}

template <bool SLOT>
__global__ __launch_bounds__(RL_EMIT) void k_rlines_emit(const DevContig* __restrict__ contigs, const RLinesDesc* __restrict__ desc, uint32_t n_desc,
                                                         const RLinesMember* __restrict__ members, const uint32_t* __restrict__ loc,
                                                         const unsigned long long* __restrict__ bbase, uint32_t n_blocks, unsigned long long* __restrict__ off,
                                                         uint64_t n_lines, char* __restrict__ out, uint64_t cap) {
    __shared__ uint4 s_stage[RL_STAGE / 16];
    __shared__ uint32_t s_start[RL_MAX_LPW + 1];
    const uint32_t e = blockIdx.x, lane = threadIdx.x;
    const RLinesDesc d = desc[rlines_desc_of_emit(desc, n_desc, e)];
    const uint32_t l0 = (e - d.eblk0) * d.lpw;                       // the wave's first line (lpw divides RL_BLOCK: all in one block of the scan)
    const uint32_t n = d.R - l0 < d.lpw ? d.R - l0 : d.lpw;
    const uint32_t blk = d.blk0 + l0 / RL_BLOCK;
    const uint64_t base = bbase[blk];
    const uint32_t B = (uint32_t)(bbase[blk + 1] - base);
    for (uint32_t i = lane; i <= n; i += RL_EMIT) {
        const uint32_t l = l0 + i;
        const bool here = i < n || (l < d.R && l % RL_BLOCK != 0u);  // (the line behind the wave's, if the block has one)
        const uint32_t start = here ? loc[d.line0 + l] : B;
        s_start[i] = start;
        if (i < n) off[d.line0 + l] = base + start;
    }
    if (e == gridDim.x - 1 && lane == 0) off[n_lines] = bbase[n_blocks];
    __syncthreads();
    const uint32_t first = s_start[0];
    if (s_start[n] == first) return;   // (every line the host's: whole waves leave)
    unsigned char* stage = (unsigned char*)s_stage;
    uint64_t gpos = base + first;
    uint32_t shift = (uint32_t)(gpos & 15u), fill = shift;
    constexpr uint32_t H = SLOT ? 3u : 1u;       // pieces of a line: the prefix (SLOT: head, number, tail), the members' texts, the newline
    const uint32_t P = d.S + H + 1u, Q = n * P;
    for (uint32_t q0 = 0; q0 < Q; q0 += RL_EMIT) {
        const uint32_t q = q0 + lane;
        const char* src = nullptr;
        uint32_t tot = 0, lead = 0;     // lead: the character in front of the piece's bytes, 0 for none
        uint64_t digits = 0;            // the number piece has no source: its characters, the first in the lowest byte
        bool number = false;
        if (q < Q) {
            const uint32_t ll = q / P, p = q - ll * P, r = l0 + ll;
            if (s_start[ll + 1] != s_start[ll]) {
                if (p < H) {
                    const uint64_t o = d.prefix_off[r];
                    const uint32_t len = (uint32_t)(d.prefix_off[r + 1] - o);
                    if constexpr (SLOT) {
                        const uint32_t sl = d.slot ? d.slot[r] : len;   // (no slots: the head is the prefix, number and tail are empty)
                        if (p == 0u) {
                            src = d.prefix + o;
                            tot = sl;
                        } else if (p == 2u) {
                            src = d.prefix + o + sl;
                            tot = len - sl;
                        } else if (d.slot) {
                            const uint32_t uk = rlines_uk(contigs, d, r);
                            digits = rlines_chars(uk);
                            tot = rlines_digits(uk);
                            number = true;
                        }
                    } else {
                        src = d.prefix + o;
                        tot = len;
                    }
                } else if (p < d.S + H) {
                    const RLinesMember m = members[d.mem0 + p - H];
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
        const bool big = tot > RL_SMALL;
        const unsigned long long bigmask = __ballot(big);
        const uint32_t nl = lead ? 1u : 0u;
        uint32_t done = 0;
        while (done < T) {   // the step's T bytes, window by window
            const uint32_t room = RL_STAGE - fill, w = T - done < room ? T - done : room, w1 = done + w;
            if (!big) {
                const uint32_t x0 = a > done ? a : done, x1 = a + tot < w1 ? a + tot : w1;
                for (uint32_t x = x0; x < x1; ++x) {
                    unsigned char ch;
                    if (SLOT && number) ch = (unsigned char)(digits >> (8u * (x - a)));
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
                for (uint32_t x = y0 + lane; x < y1; x += RL_EMIT) stage[fill + (x - done)] = nj && x == aj ? (unsigned char)leadj : (unsigned char)srcj[x - aj - nj];
            }
            fill += w;
            done = w1;
            if (fill == RL_STAGE) {
                __syncthreads();
                rtext_flush<RL_EMIT>(s_stage, out, gpos - shift, shift, fill, cap, lane);
                __syncthreads();
                gpos += fill - shift;   // (a multiple of 16 from here on)
                shift = 0;
                fill = 0;
            }
        }
    }
    __syncthreads();
    if (fill > shift) rtext_flush<RL_EMIT>(s_stage, out, gpos - shift, shift, fill, cap, lane);
}

template <bool SLOT>
void rlines_launch(const DevContig* d_contigs, const RLinesDesc* d_desc, uint32_t n_desc, const RLinesMember* d_members, uint32_t n_blocks,
                   uint32_t n_emit_blocks, uint32_t* d_loc, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off, uint64_t n_lines, char* d_out, uint64_t cap,
                   hipStream_t s) {
    hipLaunchKernelGGL(k_rlines_len<SLOT>, dim3(n_blocks), dim3(RL_BLOCK), 0, s, d_contigs, d_desc, n_desc, d_members, d_loc, d_bsum);
    hipLaunchKernelGGL(k_rlines_sums, dim3(1), dim3(RL_BLOCK), 0, s, d_bsum, n_blocks, (unsigned long long*)d_bbase);
    hipLaunchKernelGGL(k_rlines_emit<SLOT>, dim3(n_emit_blocks), dim3(RL_EMIT), 0, s, d_contigs, d_desc, n_desc, d_members, d_loc,
                       (const unsigned long long*)d_bbase, n_blocks, (unsigned long long*)d_off, n_lines, d_out, cap);
}

}  // namespace

extern "C" uint32_t pgk_rlines_block(void) { return RL_BLOCK; }
extern "C" uint32_t pgk_rlines_stage_bytes(void) { return RL_STAGE; }
// lines per wave of k_rlines_emit for S members: the largest power of two with at most RL_MAX_PIECES pieces of S + 2 a line
// (slotted: RL_MAX_PIECES_SLOT of S + 4), at least 1 and at most 64
extern "C" uint32_t pgk_rlines_lines_per_wave(uint32_t n_members, bool slotted) {
    const uint64_t per_line = (uint64_t)n_members + (slotted ? 4u : 2u), most = slotted ? RL_MAX_PIECES_SLOT : RL_MAX_PIECES;
    uint32_t lpw = RL_MAX_LPW;
    while (lpw > 1u && (uint64_t)lpw * per_line > most) lpw >>= 1;
    return lpw;
}

extern "C" void pgk_launch_rlines(const DevContig* d_contigs, const RLinesDesc* d_desc, uint32_t n_desc, const RLinesMember* d_members, bool slotted,
                                  uint32_t n_blocks, uint32_t n_emit_blocks, uint32_t* d_loc, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off,
                                  uint64_t n_lines, char* d_out, uint64_t cap, hipStream_t s) {
    if (!n_desc || !n_blocks || !n_emit_blocks) return;
    if (slotted) rlines_launch<true>(d_contigs, d_desc, n_desc, d_members, n_blocks, n_emit_blocks, d_loc, d_bsum, d_bbase, d_off, n_lines, d_out, cap, s);
    else rlines_launch<false>(d_contigs, d_desc, n_desc, d_members, n_blocks, n_emit_blocks, d_loc, d_bsum, d_bbase, d_off, n_lines, d_out, cap, s);
}
