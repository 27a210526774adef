// pg_calls_dev.h — the device helpers the kernels of pg_calls.hip and pg_combine.hip share: the 8-byte record of a call
// and the order in which the wave-per-variant kernels pick the likeliest genotype.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_calls.h"

__device__ __forceinline__ static unsigned long long pack_call(uint32_t a1, uint32_t a2, uint32_t gq, uint32_t flags) {
    return (unsigned long long)(a1 & 0xFFFFu) | ((unsigned long long)(a2 & 0xFFFFu) << 16) | ((unsigned long long)(gq & 0xFFFFu) << 32) |
           ((unsigned long long)(flags & 0xFFFFu) << 48);
}
__device__ __forceinline__ static unsigned long long pack_no_call(uint32_t flags) { return pack_call(0xFFFFu, 0xFFFFu, 0u, flags); }

// (value, bin) pairs ordered by value, then by bin: the reference's `>=` keeps the LAST of equal maxima
__device__ __forceinline__ static bool wide_better(pgx q, uint32_t bin, pgx best, uint32_t best_bin) {
    const int c = pgx_cmp(q, best);
    return c > 0 || (c == 0 && bin > best_bin);
}
