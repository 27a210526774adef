// pg_text_scan.h — the device helpers the units of packed text share (pg_record_text.hip: the bytes of a sample column;
// pg_record_lines.hip: whole VCF lines, over plain and slotted prefixes): the wave scan, the block scan, the scan of the
// block sums and the flush of an LDS stage to its contiguous byte range.  Device code only; each unit keeps
// its own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PGT_BLOCK 256                 // threads of a scanning block: one length each
#define PGT_WAVES (PGT_BLOCK / 64)

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// The lengths of a block's PGT_BLOCK threads: returns the bytes of the threads before this one, *total = the block's bytes.
// s_wave: PGT_WAVES words of LDS.  Every thread of the block calls it.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t len, uint32_t* s_wave, uint32_t* total) {
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    const uint32_t incl = wave_incl_scan(len, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (uint32_t w = 0; w < PGT_WAVES; ++w) {
        const uint32_t x = s_wave[w];
        if (w < wave) before += x;
        sum += x;
    }
    *total = sum;
    return before + incl - len;
}

// bbase[b] = the bytes of the blocks before b, b = 0 .. n, in 64 bits (one workgroup of PGT_BLOCK threads: n is a 256th of
// the lengths).  s_wave: PGT_WAVES 64-bit words of LDS.
__device__ __forceinline__ void block_sums_scan(const uint32_t* __restrict__ bsum, uint32_t n, unsigned long long* __restrict__ bbase,
                                                unsigned long long* s_wave) {
    const uint32_t tid = threadIdx.x, lane = tid % 64u, wave = tid / 64u;
    unsigned long long carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += PGT_BLOCK) {
        const uint32_t b = b0 + tid;
        const unsigned long long x = b < n ? bsum[b] : 0ull;
        unsigned long long incl = x;
        for (uint32_t dd = 1; dd < 64; dd <<= 1) {
            const unsigned long long y = __shfl_up(incl, dd, 64);
            if (lane >= dd) incl += y;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (uint32_t w = 0; w < PGT_WAVES; ++w) {
            const unsigned long long y = s_wave[w];
            if (w < wave) before += y;
            total += y;
        }
        if (b < n) bbase[b] = carry + before + incl - x;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) bbase[n] = carry;
}

// Bytes [lo, hi) of the stage to text[g16 + lo .. g16 + hi), g16 a multiple of 16: chunk c of the stage is chunk c of the
// range.  Whole chunks as one 16-byte store, the two ends as bytes; nothing at or behind `cap`.
template <uint32_t NT>
__device__ __forceinline__ void rtext_flush(const uint4* __restrict__ stage4, char* __restrict__ text, uint64_t g16, uint32_t lo, uint32_t hi, uint64_t cap,
                                            uint32_t tid) {
    const unsigned char* stage = (const unsigned char*)stage4;
    const uint32_t c1 = (hi + 15u) / 16u;
    for (uint32_t c = lo / 16u + tid; c < c1; c += NT) {
        const uint32_t b0 = c * 16u;
        const uint64_t g = g16 + b0;
        if (b0 >= lo && b0 + 16u <= hi && g + 16u <= cap) *(uint4*)(text + g) = stage4[c];
        else {
            const uint32_t x0 = b0 > lo ? b0 : lo, x1 = b0 + 16u < hi ? b0 + 16u : hi;
            for (uint32_t x = x0; x < x1; ++x)
                if (g16 + x < cap) text[g16 + x] = (char)stage[x];
        }
    }
}
