// pg_kmers.hip — the device k-mer counter of include/pangenie_kmers.h: TargetedKmerCounter
// (pangenie_amd/host/kmer_counts.cpp) with the table in HBM.  gfx950.
//
// A workgroup of KK_BLOCK lanes takes KK_TILE = 16 * KK_BLOCK text positions plus a halo of two 16-byte chunks (k - 1 <= 31
// letters): lane t loads chunk t with one 16-byte load and packs it to 2 bits a letter and one validity bit a letter in LDS.
// Lane t then owns the 16 windows that START in chunk t: it reads chunks t, t+1, t+2 (96 + 48 bits), rolls forward and reverse
// code over them as the host does and keeps the canonical codes of its whole windows in registers.
//   kk_count:    one slot load per window, all 16 issued before the first is looked at; windows that met a foreign key go
//                round again together; a hit is one no-return 64-bit atomic add at agent scope, issued after the last round.
//   kk_register: the same codes appended to the list of registered codes (one cursor add per workgroup).
//   kk_insert:   builds the table from that list with compare-and-swap on the key.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/pangenie_counts.h"
#include "../../include/pangenie_kmers.h"
#include "pg_device.h"

#define KK_BLOCK 256
#define KK_WPL 16                     // windows per lane = letters per 16-byte chunk
#define KK_TILE (KK_BLOCK * KK_WPL)   // text positions per workgroup
#define KK_EMPTY (~0ull)
#define KK_STAGES 3
#define KK_STAGE_BYTES ((size_t)8 << 20)
#define KK_PAD 64                     // bytes behind a device text: the last chunk load of a text stays inside its buffer

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? PG_ERR_NOMEM : PG_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
}
#define KK_TRY(call)                                          \
    do {                                                      \
        const hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #call);     \
    } while (0)

struct Slot { unsigned long long key, count; };

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {   // splitmix64 finaliser, as kmer_counts.cpp
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
    return x;
}
__device__ __forceinline__ uint64_t slot_of(uint64_t code, uint64_t cap) { return __umul64hi(mix64(code), cap); }

// 16 bytes of text -> 16 x 2 bits (letter i at bits 2i) and 16 validity bits; positions at or behind `left` are not text
__device__ __forceinline__ void pack_chunk(const uint4 raw, uint64_t left, uint32_t& codes, uint32_t& valid) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    codes = 0; valid = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        const uint32_t u = c & 0xDFu;                       // upper case of a letter; no other byte maps onto A, C, G, T
        const uint32_t ok = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T');
        const uint32_t two = (c >> 1) & 3u;                 // A 0, C 1, T 2, G 3
        codes |= (two ^ (two >> 1)) << (2 * i);             // A 0, C 1, G 2, T 3
        valid |= (ok & (uint32_t)((uint64_t)i < left)) << i;
    }
}

// Canonical codes of the 16 windows that start in this lane's chunk: code[j] for window j, bit j of the result set when
// the window is whole.  All lanes of the workgroup must call (barrier inside).
__device__ __forceinline__ uint32_t tile_codes(const char* __restrict__ text, uint64_t bytes, uint32_t k, uint64_t (&code)[KK_WPL]) {
    __shared__ uint32_t s_codes[KK_BLOCK + 2], s_valid[KK_BLOCK + 2];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * KK_TILE;
    for (uint32_t c = t; c < KK_BLOCK + 2; c += KK_BLOCK) {   // (lanes 0 and 1 take the halo chunks too)
        const uint64_t at = base + (uint64_t)c * 16;
        uint32_t cw = 0, vw = 0;
        if (at < bytes) pack_chunk(*reinterpret_cast<const uint4*>(text + at), bytes - at, cw, vw);
        s_codes[c] = cw;
        s_valid[c] = vw;
    }
    __syncthreads();
    uint64_t lo = (uint64_t)s_codes[t] | ((uint64_t)s_codes[t + 1] << 32), hi = s_codes[t + 2];
    uint64_t ok = (uint64_t)s_valid[t] | ((uint64_t)s_valid[t + 1] << 16) | ((uint64_t)s_valid[t + 2] << 32);
    const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
    const uint32_t top = 2 * (k - 1);
    uint64_t fwd = 0, rev = 0;
    uint32_t filled = 0, whole = 0;
    auto step = [&]() {
        const uint64_t b = lo & 3ull;
        fwd = ((fwd << 2) | b) & mask;
        rev = (rev >> 2) | ((3ull - b) << top);
        filled = (ok & 1ull) ? filled + 1 : 0;
        lo = (lo >> 2) | (hi << 62); hi >>= 2; ok >>= 1;
    };
    for (uint32_t m = 0; m + 1 < k; ++m) step();
#pragma unroll
    for (int j = 0; j < KK_WPL; ++j) {
        step();
        code[j] = fwd < rev ? fwd : rev;
        whole |= (uint32_t)(filled >= k) << j;
    }
    return whole;
}

__global__ __launch_bounds__(KK_BLOCK) void kk_count(const char* __restrict__ text, uint64_t bytes, uint32_t k,
                                                     Slot* __restrict__ slots, uint64_t cap, unsigned long long* __restrict__ windows) {
    __shared__ uint32_t s_seen;
    if (threadIdx.x == 0) s_seen = 0;
    uint64_t code[KK_WPL];
    uint32_t todo = tile_codes(text, bytes, k, code);   // (its barrier orders s_seen = 0 too)
    if (todo) atomicAdd(&s_seen, (uint32_t)__popc(todo));
    __syncthreads();   // (before the probes: a barrier behind them would wait for every atomic of the wave)
    if (threadIdx.x == 0 && s_seen) (void)__hip_atomic_fetch_add(windows, (unsigned long long)s_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint64_t at[KK_WPL], key[KK_WPL];
    // first probe of all 16 windows, whole or not (a slot index is always inside the table): 16 independent loads in flight
#pragma unroll
    for (int j = 0; j < KK_WPL; ++j) at[j] = slot_of(code[j], cap);
#pragma unroll
    for (int j = 0; j < KK_WPL; ++j) key[j] = slots[at[j]].key;
    // Rounds: all keys of a round are looked at before anything else is issued; the windows that met a foreign key look at
    // the next slot together.  The increments wait until the last round: an atomic between two rounds would stand in front
    // of the next round's loads in the wave's memory counter, and the round would wait for it.
    uint32_t hits = 0;
    while (true) {
        uint32_t more = 0;
#pragma unroll
        for (int j = 0; j < KK_WPL; ++j) {
            const uint32_t open = (todo >> j) & 1u;
            hits |= (open & (uint32_t)(key[j] == code[j])) << j;
            more |= (open & (uint32_t)(key[j] != code[j] && key[j] != KK_EMPTY)) << j;
        }
        todo = more;
        if (!todo) break;
#pragma unroll
        for (int j = 0; j < KK_WPL; ++j)
            if ((todo >> j) & 1u) {
                at[j] = at[j] + 1 == cap ? 0 : at[j] + 1;
                key[j] = slots[at[j]].key;
            }
    }
#pragma unroll
    for (int j = 0; j < KK_WPL; ++j)
        if ((hits >> j) & 1u) (void)__hip_atomic_fetch_add(&slots[at[j]].count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ctr[0] = cursor into `out` (codes registered so far), ctr[1] = set when `out` was too small (nothing is written then)
__global__ __launch_bounds__(KK_BLOCK) void kk_register(const char* __restrict__ text, uint64_t bytes, uint32_t k,
                                                        unsigned long long* __restrict__ out, uint64_t out_cap, unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t s_wave[KK_BLOCK / 64];
    __shared__ unsigned long long s_base;
    uint64_t code[KK_WPL];
    const uint32_t whole = tile_codes(text, bytes, k, code);
    const uint32_t mine = (uint32_t)__popc(whole), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= (uint32_t)d) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < KK_BLOCK / 64; ++w) total += s_wave[w];
        unsigned long long b = KK_EMPTY;
        if (total) {
            b = __hip_atomic_fetch_add(&ctr[0], (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b + total > out_cap) { ctr[1] = 1; b = KK_EMPTY; }
        }
        s_base = b;
    }
    __syncthreads();
    if (s_base == KK_EMPTY) return;
    uint64_t to = s_base + incl - mine;
    for (uint32_t w = 0; w < wave; ++w) to += s_wave[w];
#pragma unroll
    for (int j = 0; j < KK_WPL; ++j)
        if ((whole >> j) & 1u) out[to++] = code[j];
}

__global__ void kk_fill(Slot* slots, uint64_t cap) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) slots[i] = Slot{KK_EMPTY, 0ull};
}
__global__ void kk_clear(Slot* slots, uint64_t cap) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) slots[i].count = 0ull;
}
// insert-only linear probing: compare-and-swap on the key, nothing more (TargetedKmerCounter::freeze)
__global__ void kk_insert(const unsigned long long* __restrict__ codes, uint64_t n, Slot* slots, uint64_t cap, unsigned long long* distinct) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long code = codes[i];
        uint64_t at = slot_of(code, cap);
        while (true) {
            unsigned long long seen = __hip_atomic_load(&slots[at].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == code) break;
            if (seen == KK_EMPTY) {
                if (__hip_atomic_compare_exchange_strong(&slots[at].key, &seen, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    atomicAdd(distinct, 1ull);
                    break;
                }
                if (seen == code) break;   // (another lane put the same code here first)
            }
            if (++at == cap) at = 0;
        }
    }
}
__global__ void kk_lookup(const unsigned long long* __restrict__ codes, uint64_t n, const Slot* __restrict__ slots, uint64_t cap,
                          unsigned long long* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long code = codes[i];
    unsigned long long answer = KK_EMPTY;
    if (code != KK_EMPTY) {
        uint64_t at = slot_of(code, cap);
        while (true) {
            const Slot s = slots[at];
            if (s.key == code) { answer = s.count; break; }
            if (s.key == KK_EMPTY) break;
            if (++at == cap) at = 0;
        }
    }
    counts[i] = answer;
}
#define KK_HIST_LDS 1024
__global__ __launch_bounds__(256) void kk_histogram(const Slot* __restrict__ slots, uint64_t cap, uint64_t max_count, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_h[KK_HIST_LDS];   // counts below KK_HIST_LDS meet in LDS first (a block sees far fewer than 2^32 slots)
    for (uint32_t i = threadIdx.x; i < KK_HIST_LDS; i += blockDim.x) s_h[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
        const Slot s = slots[i];
        if (s.key == KK_EMPTY || s.count == 0 || s.count > max_count) continue;
        if (s.count < KK_HIST_LDS) atomicAdd(&s_h[(uint32_t)s.count], 1u);
        else atomicAdd(&hist[s.count], 1ull);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < KK_HIST_LDS; i += blockDim.x)
        if (s_h[i]) atomicAdd(&hist[i], (unsigned long long)s_h[i]);
}

// ---------------------------------------------------------------------------------------------------- the count plan
// (include/pangenie_counts.h).  Index level, once: kk_plan_resolve turns every code the index asks about into the index
// of its slot.  Sample level: kk_plan_fill gathers the counts of those slots — no probing, no key is compared.
#define KP_BLOCK 256
#define KP_ROW 16                        // lanes that share a variant's flanking k-mers
#define KP_ROWS (KP_BLOCK / KP_ROW)      // variants per workgroup of the coverage part
template <class I> struct PlanIdx;
template <> struct PlanIdx<uint32_t> { static constexpr uint32_t none = 0xFFFFFFFFu; };
template <> struct PlanIdx<uint64_t> { static constexpr uint64_t none = ~0ull; };

// One entry per contig and one behind the last (its k_blk0 / c_blk0 = the totals).  Blocks [0, k blocks) of the grid
// take 256 unique k-mers each, the blocks behind them 16 variants each; a block finds its contig by bisection.
struct PlanDesc {
    uint64_t k_base;       // first entry of the contig in the list of unique k-mer slots
    uint64_t v_base;       // first variant of the contig in the list of flank offsets
    uint32_t k_blk0, c_blk0;
    uint32_t n_k, n_v;
    uint16_t* out_k;
    uint16_t* out_c;
};

// ctr[0] = valid codes that are not in the table, ctr[1] = the smallest `first + i` among them
template <class I>
__global__ __launch_bounds__(KP_BLOCK) void kk_plan_resolve(const unsigned long long* __restrict__ codes, uint64_t n, uint64_t first,
                                                            const Slot* __restrict__ slots, uint64_t cap, I* __restrict__ idx,
                                                            unsigned long long* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * KP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long code = codes[i];
    I answer = PlanIdx<I>::none;
    if (code != KK_EMPTY) {   // (a k-mer with a letter outside ACGT: no slot, counts 0)
        uint64_t at = slot_of(code, cap);
        while (true) {
            const unsigned long long key = slots[at].key;
            if (key == code) { answer = (I)at; break; }
            if (key == KK_EMPTY) break;
            if (++at == cap) at = 0;
        }
        if (answer == PlanIdx<I>::none) {
            atomicAdd(&ctr[0], 1ull);
            atomicMin(&ctr[1], (unsigned long long)(first + i));
        }
    }
    idx[i] = answer;
}

__device__ __forceinline__ uint32_t plan_contig_of(const PlanDesc* __restrict__ desc, uint32_t n_contigs, uint32_t block, bool cov) {
    uint32_t lo = 0, hi = n_contigs;   // the last contig whose first block is not behind `block` (empty contigs share their successor's)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((cov ? desc[mid].c_blk0 : desc[mid].k_blk0) <= block) lo = mid; else hi = mid;
    }
    return lo;
}

// One launch per sample for all contigs.  Unique k-mers: a lane per k-mer, one 8-byte load of the slot's count, 2-byte
// stores side by side.  Coverage: a row of 16 lanes per variant — the row reads 16 consecutive slot indices (one 64-byte
// piece) and has 16 gathers in flight, then sums over the row by shuffles; lists are a few dozen entries, so a lane per
// variant would walk its list alone, index after index, with every lane of the wave in a different 64-byte piece.
template <class I>
__global__ __launch_bounds__(KP_BLOCK) void kk_plan_fill(const PlanDesc* __restrict__ desc, uint32_t n_contigs, uint32_t k_blocks,
                                                         const I* __restrict__ kidx, const I* __restrict__ fidx,
                                                         const unsigned long long* __restrict__ foff, const Slot* __restrict__ slots,
                                                         uint64_t kmer_coverage) {
    const uint32_t b = blockIdx.x;
    if (b < k_blocks) {
        const PlanDesc d = desc[plan_contig_of(desc, n_contigs, b, false)];
        const uint64_t i = (uint64_t)(b - d.k_blk0) * KP_BLOCK + threadIdx.x;
        if (i >= d.n_k) return;
        const I at = kidx[d.k_base + i];
        const unsigned long long count = at == PlanIdx<I>::none ? 0ull : slots[at].count;
        d.out_k[i] = (uint16_t)count;   // (the cast of update_readcount(i, (unsigned short)...): it truncates)
        return;
    }
    const uint32_t cb = b - k_blocks;
    const PlanDesc d = desc[plan_contig_of(desc, n_contigs, cb, true)];
    const uint32_t v = (cb - d.c_blk0) * KP_ROWS + threadIdx.x / KP_ROW, lane = threadIdx.x % KP_ROW;
    if (v >= d.n_v) return;   // (whole rows leave: the shuffles below stay inside a row)
    const uint64_t lo = foff[d.v_base + v], hi = foff[d.v_base + v + 1];
    const uint64_t lowest = kmer_coverage / 4, highest = kmer_coverage * 4;
    unsigned long long sum = 0, used = 0;
    for (uint64_t j = lo + lane; j < hi; j += KP_ROW) {
        const I at = fidx[j];
        const unsigned long long count = at == PlanIdx<I>::none ? 0ull : slots[at].count;
        if (count >= lowest && count <= highest) { sum += count; used += 1; }
    }
#pragma unroll
    for (int m = KP_ROW / 2; m > 0; m >>= 1) {
        sum += __shfl_xor(sum, m, KP_ROW);
        used += __shfl_xor(used, m, KP_ROW);
    }
    if (lane == 0) d.out_c[v] = (uint16_t)((used && sum) ? sum / used : kmer_coverage);
}

struct Stage {
    char* host = nullptr;   // pinned
    char* dev = nullptr;    // KK_STAGE_BYTES + KK_PAD
    hipEvent_t done = nullptr;
    bool in_flight = false;
};

}  // namespace

struct pg_kmer_counter {
    uint32_t k = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    unsigned long long* pending = nullptr;   // device: codes registered before the table is built
    uint64_t pend_n = 0, pend_cap = 0;
    Slot* slots = nullptr;
    uint64_t cap = 0, targets = 0;
    unsigned long long* ctr = nullptr;       // device: [0] register cursor, [1] register overflow, [2] distinct, [3] windows seen
    bool frozen = false;
    Stage stage[KK_STAGES];
    bool staged = false;
    int next = 0, out = -1;                  // next staging buffer to hand out; the one handed out by acquire
};

namespace {

int use(pg_kmer_counter* h) {
    if (!h) return fail(PG_ERR_INVALID, "pg_kmer_counter: null handle");
    KK_TRY(hipSetDevice(h->device));
    return PG_OK;
}
uint32_t grid_for(uint64_t n, uint32_t block) { return (uint32_t)std::min<uint64_t>((n + block - 1) / block, 256u * 32u); }

int ensure_stages(pg_kmer_counter* h) {
    if (h->staged) return PG_OK;
    for (Stage& s : h->stage) {
        KK_TRY(hipHostMalloc((void**)&s.host, KK_STAGE_BYTES, hipHostMallocDefault));
        KK_TRY(hipMalloc((void**)&s.dev, KK_STAGE_BYTES + KK_PAD));
        KK_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    h->staged = true;
    return PG_OK;
}
int ensure_pending(pg_kmer_counter* h, uint64_t room) {
    if (h->pend_n + room <= h->pend_cap) return PG_OK;
    const uint64_t want = std::max<uint64_t>(h->pend_n + room, std::max<uint64_t>(2 * h->pend_cap, 1u << 16));
    unsigned long long* grown = nullptr;
    KK_TRY(hipMalloc((void**)&grown, want * sizeof(unsigned long long)));
    if (h->pend_n) {
        const hipError_t e = hipMemcpyAsync(grown, h->pending, h->pend_n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
        if (e2 != hipSuccess) { (void)hipFree(grown); return hip_fail(e2, "growing the list of registered codes"); }
    }
    if (h->pending) (void)hipFree(h->pending);
    h->pending = grown;
    h->pend_cap = want;
    return PG_OK;
}
int wait_stage(Stage& s) {
    if (s.in_flight) { KK_TRY(hipEventSynchronize(s.done)); s.in_flight = false; }
    return PG_OK;
}
// the text in stage `i` (its first `bytes` bytes) goes to the device and through kk_count / kk_register
int submit_stage(pg_kmer_counter* h, int i, uint64_t bytes, bool registering) {
    Stage& s = h->stage[i];
    if (bytes >= h->k) {
        KK_TRY(hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, h->stream));
        const uint32_t tiles = (uint32_t)((bytes + KK_TILE - 1) / KK_TILE);
        if (registering) hipLaunchKernelGGL(kk_register, dim3(tiles), dim3(KK_BLOCK), 0, h->stream, s.dev, bytes, h->k, h->pending, h->pend_cap, h->ctr);
        else hipLaunchKernelGGL(kk_count, dim3(tiles), dim3(KK_BLOCK), 0, h->stream, s.dev, bytes, h->k, h->slots, h->cap, h->ctr + 3);
        KK_TRY(hipGetLastError());
        KK_TRY(hipEventRecord(s.done, h->stream));
        s.in_flight = true;
    }
    return PG_OK;
}
// a host text of any length through the staging buffers: pieces overlap by k - 1 bytes, so that every window lies in
// exactly one piece as a whole window
int stream_text(pg_kmer_counter* h, const char* text, uint64_t bytes, bool registering) {
    if (int rc = ensure_stages(h)) return rc;
    const uint64_t k = h->k;
    uint64_t from = 0;
    while (from + k <= bytes) {
        const uint64_t n = std::min<uint64_t>(bytes - from, KK_STAGE_BYTES);
        const int i = h->next;
        h->next = (h->next + 1) % KK_STAGES;
        if (int rc = wait_stage(h->stage[i])) return rc;
        if (registering) {
            if (int rc = ensure_pending(h, n)) return rc;   // (a text of n bytes holds fewer than n windows)
        }
        memcpy(h->stage[i].host, text + from, n);
        if (int rc = submit_stage(h, i, n, registering)) return rc;
        if (registering) {   // the cursor is the length of the list: the next piece's room is planned from it
            unsigned long long c[2] = {0, 0};
            KK_TRY(hipMemcpyAsync(c, h->ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
            KK_TRY(hipStreamSynchronize(h->stream));
            h->stage[i].in_flight = false;
            if (c[1] || c[0] > h->pend_cap) return fail(PG_ERR_DEVICE, "pg_kmer_counter_add_text: the list of registered codes overflowed");
            h->pend_n = c[0];
        }
        if (from + n >= bytes) break;
        from += n - (k - 1);
    }
    return PG_OK;
}
int sync_all(pg_kmer_counter* h) {
    KK_TRY(hipStreamSynchronize(h->stream));
    for (Stage& s : h->stage) s.in_flight = false;
    return PG_OK;
}
int read_ctr(pg_kmer_counter* h, int which, uint64_t* value) {
    unsigned long long v = 0;
    KK_TRY(hipMemcpyAsync(&v, h->ctr + which, sizeof v, hipMemcpyDeviceToHost, h->stream));
    KK_TRY(hipStreamSynchronize(h->stream));
    *value = v;
    return PG_OK;
}
int busy(pg_kmer_counter* h, const char* who) {
    return h->out >= 0 ? fail(PG_ERR_INVALID, "%s: a staging buffer is handed out (pg_kmer_counter_submit it first)", who) : PG_OK;
}

}  // namespace

extern "C" {

const char* pg_kmer_last_error(void) { return g_err; }
uint32_t pg_kmer_tile_bytes(void) { return KK_TILE; }

int pg_kmer_counter_new(uint32_t k, int device, pg_kmer_counter** out) {
    if (!out) return fail(PG_ERR_INVALID, "pg_kmer_counter_new: null out");
    *out = nullptr;
    if (k < 1 || k > 32) return fail(PG_ERR_INVALID, "pg_kmer_counter_new: k-mer size must be 1..32, got %u", k);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return fail(PG_ERR_DEVICE, "no HIP device available (no CPU fallback)"); }
    if (device < 0 || device >= ndev) return fail(PG_ERR_INVALID, "pg_kmer_counter_new: device %d of %d", device, ndev);
    pg_kmer_counter* h = new (std::nothrow) pg_kmer_counter;
    if (!h) return fail(PG_ERR_NOMEM, "pg_kmer_counter_new: out of host memory");
    h->k = k;
    h->device = device;
    int rc = PG_OK;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->ctr, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(h->ctr, 0, 4 * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { rc = hip_fail(e, "pg_kmer_counter_new"); pg_kmer_counter_destroy(h); return rc; }
    *out = h;
    return PG_OK;
}

int pg_kmer_counter_destroy(pg_kmer_counter* h) {
    if (!h) return PG_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (Stage& s : h->stage) {
        if (s.host) (void)hipHostFree(s.host);
        if (s.dev) (void)hipFree(s.dev);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    if (h->pending) (void)hipFree(h->pending);
    if (h->slots) (void)hipFree(h->slots);
    if (h->ctr) (void)hipFree(h->ctr);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return PG_OK;
}

int pg_kmer_counter_add_codes(pg_kmer_counter* h, const uint64_t* codes, uint64_t n) {
    if (int rc = use(h)) return rc;
    if (h->frozen) return fail(PG_ERR_INVALID, "pg_kmer_counter_add_codes: targets must be registered before the reads are counted");
    if (n == 0) return PG_OK;
    if (!codes) return fail(PG_ERR_INVALID, "pg_kmer_counter_add_codes: null codes");
    if (h->k < 32) {
        const uint64_t limit = 1ull << (2 * h->k);
        for (uint64_t i = 0; i < n; ++i)
            if (codes[i] >= limit) return fail(PG_ERR_INVALID, "pg_kmer_counter_add_codes: code %llu at %llu is no %u-mer", (unsigned long long)codes[i], (unsigned long long)i, h->k);
    } else {
        for (uint64_t i = 0; i < n; ++i)
            if (codes[i] == KK_EMPTY) return fail(PG_ERR_INVALID, "pg_kmer_counter_add_codes: code at %llu is not canonical", (unsigned long long)i);
    }
    if (int rc = ensure_pending(h, n)) return rc;
    KK_TRY(hipMemcpyAsync(h->pending + h->pend_n, codes, n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    h->pend_n += n;
    const unsigned long long cursor = h->pend_n;
    KK_TRY(hipMemcpyAsync(h->ctr, &cursor, sizeof cursor, hipMemcpyHostToDevice, h->stream));
    KK_TRY(hipStreamSynchronize(h->stream));   // (the caller's array and `cursor` are free again)
    return PG_OK;
}

int pg_kmer_counter_add_text(pg_kmer_counter* h, const char* text, uint64_t bytes, uint64_t* windows) {
    if (int rc = use(h)) return rc;
    if (h->frozen) return fail(PG_ERR_INVALID, "pg_kmer_counter_add_text: targets must be registered before the reads are counted");
    if (bytes && !text) return fail(PG_ERR_INVALID, "pg_kmer_counter_add_text: null text");
    const uint64_t before = h->pend_n;
    if (int rc = stream_text(h, text, bytes, true)) return rc;
    if (windows) *windows = h->pend_n - before;
    return PG_OK;
}

int pg_kmer_counter_freeze(pg_kmer_counter* h) {
    if (int rc = use(h)) return rc;
    if (h->frozen) return PG_OK;
    const uint64_t cap = std::max<uint64_t>(16, 2 * h->pend_n + 1);
    Slot* slots = nullptr;
    const hipError_t e = hipMalloc((void**)&slots, cap * sizeof(Slot));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? PG_ERR_NOMEM : PG_ERR_DEVICE, "pg_kmer_counter_freeze: a table of %llu slots (%llu bytes) for %llu registered codes: %s",
                    (unsigned long long)cap, (unsigned long long)(cap * sizeof(Slot)), (unsigned long long)h->pend_n, hipGetErrorString(e));
    }
    h->slots = slots;
    h->cap = cap;
    hipLaunchKernelGGL(kk_fill, dim3(grid_for(cap, 256)), dim3(256), 0, h->stream, slots, cap);
    if (h->pend_n) hipLaunchKernelGGL(kk_insert, dim3(grid_for(h->pend_n, 256)), dim3(256), 0, h->stream, h->pending, h->pend_n, slots, cap, h->ctr + 2);
    KK_TRY(hipGetLastError());
    if (int rc = read_ctr(h, 2, &h->targets)) return rc;
    if (h->pending) (void)hipFree(h->pending);
    h->pending = nullptr;
    h->pend_n = h->pend_cap = 0;
    h->frozen = true;
    return PG_OK;
}

int pg_kmer_counter_count(pg_kmer_counter* h, const char* text, uint64_t bytes) {
    if (int rc = use(h)) return rc;
    if (int rc = busy(h, "pg_kmer_counter_count")) return rc;
    if (bytes && !text) return fail(PG_ERR_INVALID, "pg_kmer_counter_count: null text");
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    return stream_text(h, text, bytes, false);
}

int pg_kmer_counter_acquire(pg_kmer_counter* h, char** buffer, uint64_t* capacity) {
    if (int rc = use(h)) return rc;
    if (!buffer || !capacity) return fail(PG_ERR_INVALID, "pg_kmer_counter_acquire: null argument");
    if (int rc = busy(h, "pg_kmer_counter_acquire")) return rc;
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    if (int rc = ensure_stages(h)) return rc;
    const int i = h->next;
    if (int rc = wait_stage(h->stage[i])) return rc;
    h->next = (h->next + 1) % KK_STAGES;
    h->out = i;
    *buffer = h->stage[i].host;
    *capacity = KK_STAGE_BYTES;
    return PG_OK;
}

int pg_kmer_counter_submit(pg_kmer_counter* h, uint64_t bytes) {
    if (int rc = use(h)) return rc;
    if (h->out < 0) return fail(PG_ERR_INVALID, "pg_kmer_counter_submit: no staging buffer is handed out");
    if (bytes > KK_STAGE_BYTES) return fail(PG_ERR_INVALID, "pg_kmer_counter_submit: %llu bytes in a buffer of %llu", (unsigned long long)bytes, (unsigned long long)KK_STAGE_BYTES);
    const int i = h->out;
    h->out = -1;
    return submit_stage(h, i, bytes, false);
}

int pg_kmer_counter_sync(pg_kmer_counter* h) {
    if (int rc = use(h)) return rc;
    return sync_all(h);
}

int pg_kmer_counter_lookup(pg_kmer_counter* h, const uint64_t* codes, uint64_t n, uint64_t* counts) {
    if (int rc = use(h)) return rc;
    if (n == 0) return PG_OK;
    if (!codes || !counts) return fail(PG_ERR_INVALID, "pg_kmer_counter_lookup: null argument");
    if (n > 0xFFFFFFFFull * 256ull) return fail(PG_ERR_UNSUPPORTED, "pg_kmer_counter_lookup: more than 2^40 codes in one call");
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    unsigned long long* d = nullptr;
    KK_TRY(hipMalloc((void**)&d, 2 * n * sizeof(unsigned long long)));
    hipError_t e = hipMemcpyAsync(d, codes, n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream);   // (behind every count on the stream)
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kk_lookup, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, h->stream, d, n, h->slots, h->cap, d + n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(counts, d + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "pg_kmer_counter_lookup");
    for (Stage& s : h->stage) s.in_flight = false;
    return PG_OK;
}

int pg_kmer_counter_stats(pg_kmer_counter* h, uint64_t* targets, uint64_t* windows) {
    if (int rc = use(h)) return rc;
    if (targets) {
        if (int rc = pg_kmer_counter_freeze(h)) return rc;
        *targets = h->targets;
    }
    if (windows) {
        if (int rc = read_ctr(h, 3, windows)) return rc;
    }
    return PG_OK;
}

int pg_kmer_counter_histogram(pg_kmer_counter* h, uint64_t max_count, uint64_t* out) {
    if (int rc = use(h)) return rc;
    if (!out) return fail(PG_ERR_INVALID, "pg_kmer_counter_histogram: null out");
    if (max_count >= ((uint64_t)1 << 28)) return fail(PG_ERR_UNSUPPORTED, "pg_kmer_counter_histogram: max_count %llu (limit 2^28 - 1)", (unsigned long long)max_count);
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    unsigned long long* d = nullptr;
    const size_t bytes = (max_count + 1) * sizeof(unsigned long long);
    KK_TRY(hipMalloc((void**)&d, bytes));
    hipError_t e = hipMemsetAsync(d, 0, bytes, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kk_histogram, dim3(grid_for(h->cap, 256 * 8)), dim3(256), 0, h->stream, h->slots, h->cap, max_count, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "pg_kmer_counter_histogram");
    return PG_OK;
}

int pg_kmer_counter_reset_counts(pg_kmer_counter* h) {
    if (int rc = use(h)) return rc;
    if (int rc = busy(h, "pg_kmer_counter_reset_counts")) return rc;
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    hipLaunchKernelGGL(kk_clear, dim3(grid_for(h->cap, 256)), dim3(256), 0, h->stream, h->slots, h->cap);
    KK_TRY(hipGetLastError());
    KK_TRY(hipMemsetAsync(h->ctr + 3, 0, sizeof(unsigned long long), h->stream));
    return sync_all(h);
}

int pg_kmer_counter_capacity(pg_kmer_counter* h, uint64_t* capacity) {
    if (int rc = use(h)) return rc;
    if (!capacity) return fail(PG_ERR_INVALID, "pg_kmer_counter_capacity: null capacity");
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    *capacity = h->cap;
    return PG_OK;
}

int pg_kmer_counter_table(pg_kmer_counter* h, uint64_t* slots, uint64_t capacity) {
    if (int rc = use(h)) return rc;
    if (!slots) return fail(PG_ERR_INVALID, "pg_kmer_counter_table: null slots");
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    if (capacity != h->cap) return fail(PG_ERR_INVALID, "pg_kmer_counter_table: room for %llu slots, the table has %llu", (unsigned long long)capacity, (unsigned long long)h->cap);
    KK_TRY(hipMemcpyAsync(slots, h->slots, h->cap * sizeof(Slot), hipMemcpyDeviceToHost, h->stream));
    return sync_all(h);
}

int pg_kmer_counter_count_resident(pg_kmer_counter* h, const char* text, uint64_t bytes, uint32_t repeats, double* ms) {
    if (int rc = use(h)) return rc;
    if (int rc = busy(h, "pg_kmer_counter_count_resident")) return rc;
    if ((bytes && !text) || (repeats && !ms)) return fail(PG_ERR_INVALID, "pg_kmer_counter_count_resident: null argument");
    if (bytes >= (uint64_t)0xFFFFFFFFu * KK_TILE) return fail(PG_ERR_UNSUPPORTED, "pg_kmer_counter_count_resident: text too long for one launch");
    if (int rc = pg_kmer_counter_freeze(h)) return rc;
    for (uint32_t r = 0; r < repeats; ++r) ms[r] = 0.0;
    if (bytes < h->k || repeats == 0) return PG_OK;
    char* d = nullptr;
    KK_TRY(hipMalloc((void**)&d, bytes + KK_PAD));
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) e = hipMemcpyAsync(d, text, bytes, hipMemcpyHostToDevice, h->stream);
    const uint32_t tiles = (uint32_t)((bytes + KK_TILE - 1) / KK_TILE);
    for (uint32_t r = 0; r < repeats && e == hipSuccess; ++r) {
        e = hipEventRecord(a, h->stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(kk_count, dim3(tiles), dim3(KK_BLOCK), 0, h->stream, d, bytes, h->k, h->slots, h->cap, h->ctr + 3);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(b, h->stream);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
        ms[r] = t;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "pg_kmer_counter_count_resident");
    return PG_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------- the count plan
struct pg_count_plan {
    pg_kmer_counter* counter = nullptr;
    bool lenient = false, wide = false;          // wide: the table has 2^32 - 1 slots or more, slot indices take 64 bits
    uint32_t nc = 0;
    std::vector<uint32_t> n_variants;            // [nc]
    std::vector<std::vector<uint32_t>> koff;     // [nc][V + 1] host copies: what pg_count_plan_fill_job compares with the job's
    std::vector<PlanDesc> desc;                  // [nc + 1]; the output pointers are set by every fill
    uint64_t n_k = 0, n_f = 0, n_v = 0, unresolved = 0, device_bytes = 0;
    uint32_t k_blocks = 0, c_blocks = 0;
    void* d_kidx = nullptr;                      // [n_k] slot of every unique k-mer, contig after contig
    void* d_fidx = nullptr;                      // [n_f] ... of every flanking k-mer
    unsigned long long* d_foff = nullptr;        // [n_v + 1] flanking k-mers of variant v (over all contigs): [d_foff[v], d_foff[v + 1])
    PlanDesc* d_desc = nullptr;
    uint16_t* d_out_k = nullptr;                 // pg_count_plan_fill_host's device arrays (allocated by its first call)
    uint16_t* d_out_c = nullptr;
    uint16_t* h_k = nullptr;                     // pinned: [n_k] (fill_host), [n_v] (fill_host, fill_job)
    uint16_t* h_c = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double last_ms = 0.0;
};

namespace {

constexpr uint64_t kPlanChunk = (uint64_t)1 << 24;   // codes resolved per launch: 128 MB of codes on the device at a time

int plan_use(pg_count_plan* p, const char* who) {
    if (!p) return fail(PG_ERR_INVALID, "%s: null plan", who);
    if (int rc = use(p->counter)) return rc;
    if (int rc = busy(p->counter, who)) return rc;
    return sync_all(p->counter);   // everything submitted is counted
}

// `n` codes of one contig's list through the resolve kernel, a chunk at a time
int plan_resolve(pg_count_plan* p, const uint64_t* codes, uint64_t n, uint64_t base, bool flanks, unsigned long long* d_codes, unsigned long long* d_ctr) {
    pg_kmer_counter* h = p->counter;
    for (uint64_t at = 0; at < n; at += kPlanChunk) {
        const uint64_t m = std::min<uint64_t>(kPlanChunk, n - at);
        KK_TRY(hipMemcpyAsync(d_codes, codes + at, m * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
        const dim3 grid((uint32_t)((m + KP_BLOCK - 1) / KP_BLOCK));
        unsigned long long* ctr = d_ctr + (flanks ? 2 : 0);
        if (p->wide) {
            uint64_t* idx = (uint64_t*)(flanks ? p->d_fidx : p->d_kidx) + base + at;
            hipLaunchKernelGGL(kk_plan_resolve<uint64_t>, grid, dim3(KP_BLOCK), 0, h->stream, d_codes, m, base + at, h->slots, h->cap, idx, ctr);
        } else {
            uint32_t* idx = (uint32_t*)(flanks ? p->d_fidx : p->d_kidx) + base + at;
            hipLaunchKernelGGL(kk_plan_resolve<uint32_t>, grid, dim3(KP_BLOCK), 0, h->stream, d_codes, m, base + at, h->slots, h->cap, idx, ctr);
        }
        KK_TRY(hipGetLastError());
        KK_TRY(hipStreamSynchronize(h->stream));   // (d_codes is free for the next chunk; a pageable source has been read)
    }
    return PG_OK;
}

// descriptors (with this fill's output pointers) to the device, the kernel between the two events
int plan_launch(pg_count_plan* p, uint64_t kmer_coverage) {
    pg_kmer_counter* h = p->counter;
    const uint32_t blocks = p->k_blocks + p->c_blocks;
    p->last_ms = 0.0;
    if (blocks == 0) return PG_OK;
    KK_TRY(hipMemcpyAsync(p->d_desc, p->desc.data(), p->desc.size() * sizeof(PlanDesc), hipMemcpyHostToDevice, h->stream));
    KK_TRY(hipEventRecord(p->ev[0], h->stream));
    if (p->wide)
        hipLaunchKernelGGL(kk_plan_fill<uint64_t>, dim3(blocks), dim3(KP_BLOCK), 0, h->stream, p->d_desc, p->nc, p->k_blocks, (const uint64_t*)p->d_kidx,
                           (const uint64_t*)p->d_fidx, p->d_foff, h->slots, kmer_coverage);
    else
        hipLaunchKernelGGL(kk_plan_fill<uint32_t>, dim3(blocks), dim3(KP_BLOCK), 0, h->stream, p->d_desc, p->nc, p->k_blocks, (const uint32_t*)p->d_kidx,
                           (const uint32_t*)p->d_fidx, p->d_foff, h->slots, kmer_coverage);
    KK_TRY(hipGetLastError());
    KK_TRY(hipEventRecord(p->ev[1], h->stream));
    return PG_OK;
}
int plan_finish(pg_count_plan* p) {
    KK_TRY(hipStreamSynchronize(p->counter->stream));
    if (p->k_blocks + p->c_blocks) {
        float ms = 0.f;
        KK_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
        p->last_ms = ms;
    }
    return PG_OK;
}

// where entry `flat` of the concatenated lists lies: contig, variant, position inside the variant's list
template <class Off>
void plan_locate(const pg_count_plan* p, const pg_count_contig* contigs, bool flanks, uint64_t flat, uint32_t* c_out, uint32_t* v_out, uint64_t* at_out) {
    uint64_t base = 0;
    for (uint32_t c = 0; c < p->nc; ++c) {
        const uint32_t V = contigs[c].n_variants;
        const Off* off = flanks ? (const Off*)(const void*)contigs[c].flank_off : (const Off*)(const void*)contigs[c].kmer_off;
        const uint64_t n = V ? (uint64_t)off[V] : 0;
        if (flat < base + n) {
            const uint64_t local = flat - base;
            const uint32_t v = (uint32_t)(std::upper_bound(off, off + V + 1, (Off)local) - off) - 1;
            *c_out = c; *v_out = v; *at_out = local - off[v];
            return;
        }
        base += n;
    }
    *c_out = *v_out = 0; *at_out = 0;
}

}  // namespace

extern "C" {

int pg_count_plan_destroy(pg_count_plan* p) {
    if (!p) return PG_OK;
    if (p->counter) (void)hipSetDevice(p->counter->device);
    if (p->counter && p->counter->stream) (void)hipStreamSynchronize(p->counter->stream);
    for (void* d : {p->d_kidx, p->d_fidx, (void*)p->d_foff, (void*)p->d_desc, (void*)p->d_out_k, (void*)p->d_out_c})
        if (d) (void)hipFree(d);
    if (p->h_k) (void)hipHostFree(p->h_k);
    if (p->h_c) (void)hipHostFree(p->h_c);
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    delete p;
    return PG_OK;
}

int pg_count_plan_new(pg_kmer_counter* counter, uint32_t n_contigs, const pg_count_contig* contigs, int unregistered_counts_zero, pg_count_plan** out) {
    if (!out) return fail(PG_ERR_INVALID, "pg_count_plan_new: null out");
    *out = nullptr;
    if (!counter) return fail(PG_ERR_INVALID, "pg_count_plan_new: null counter");
    if (n_contigs && !contigs) return fail(PG_ERR_INVALID, "pg_count_plan_new: null contigs");
    // everything the host can decide, before any device call
    const uint32_t k = counter->k;
    uint64_t n_k = 0, n_f = 0, n_v = 0, k_blocks = 0, c_blocks = 0;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const pg_count_contig& g = contigs[c];
        const uint32_t V = g.n_variants;
        uint64_t nk = 0, nf = 0;
        if (V) {
            if (!g.kmer_off || !g.flank_off) return fail(PG_ERR_INVALID, "pg_count_plan_new: contig %u has %u variants and a null offset array", c, V);
            if (g.kmer_off[0] != 0 || g.flank_off[0] != 0) return fail(PG_ERR_INVALID, "pg_count_plan_new: contig %u: offsets must start at 0", c);
            for (uint32_t v = 0; v < V; ++v)
                if (g.kmer_off[v + 1] < g.kmer_off[v] || g.flank_off[v + 1] < g.flank_off[v])
                    return fail(PG_ERR_INVALID, "pg_count_plan_new: contig %u: offsets decrease at variant %u", c, v);
            nk = g.kmer_off[V];
            nf = g.flank_off[V];
        }
        if ((nk && !g.kmer_code) || (nf && !g.flank_code)) return fail(PG_ERR_INVALID, "pg_count_plan_new: contig %u has a null code array", c);
        if (k < 32) {
            const uint64_t limit = 1ull << (2 * k);
            for (int pass = 0; pass < 2; ++pass) {
                const uint64_t* codes = pass ? g.flank_code : g.kmer_code;
                const uint64_t n = pass ? nf : nk;
                for (uint64_t i = 0; i < n; ++i)
                    if (codes[i] >= limit && codes[i] != KK_EMPTY)
                        return fail(PG_ERR_INVALID, "pg_count_plan_new: contig %u: %s code %llu at %llu is no %u-mer", c, pass ? "flanking" : "unique",
                                    (unsigned long long)codes[i], (unsigned long long)i, k);
            }
        }
        n_k += nk; n_f += nf; n_v += V;
        k_blocks += (nk + KP_BLOCK - 1) / KP_BLOCK;
        c_blocks += ((uint64_t)V + KP_ROWS - 1) / KP_ROWS;
    }
    if (k_blocks + c_blocks > 0x7FFFFFFFull) return fail(PG_ERR_UNSUPPORTED, "pg_count_plan_new: %llu k-mers and %llu variants are more than one launch takes",
                                                          (unsigned long long)n_k, (unsigned long long)n_v);
    if (int rc = use(counter)) return rc;
    if (int rc = pg_kmer_counter_freeze(counter)) return rc;
    pg_count_plan* p = new (std::nothrow) pg_count_plan;
    if (!p) return fail(PG_ERR_NOMEM, "pg_count_plan_new: out of host memory");
    p->counter = counter;
    p->lenient = unregistered_counts_zero != 0;
    p->wide = counter->cap > 0xFFFFFFFFull;   // (slot indices up to cap - 1 and the sentinel 2^32 - 1)
    // PG_COUNT_PLAN=wide (a test switch): 64-bit slot indices whatever the table's size, so that the kernels
    // of a table of 2^32 slots run on one of thousands; any other value is ignored
    if (const char* e = getenv("PG_COUNT_PLAN")) {
        if (!strcmp(e, "wide")) p->wide = true;
    }
    p->nc = n_contigs;
    p->n_k = n_k; p->n_f = n_f; p->n_v = n_v;
    p->k_blocks = (uint32_t)k_blocks; p->c_blocks = (uint32_t)c_blocks;
    p->n_variants.resize(n_contigs);
    p->koff.resize(n_contigs);
    p->desc.assign((size_t)n_contigs + 1, PlanDesc{});
    std::vector<unsigned long long> foff((size_t)n_v + 1, 0);
    {
        uint64_t kb = 0, fb = 0, vb = 0;
        uint32_t kblk = 0, cblk = 0;
        for (uint32_t c = 0; c < n_contigs; ++c) {
            const pg_count_contig& g = contigs[c];
            const uint32_t V = g.n_variants;
            p->n_variants[c] = V;
            if (V) p->koff[c].assign(g.kmer_off, g.kmer_off + V + 1);
            PlanDesc& d = p->desc[c];
            d.k_base = kb; d.v_base = vb; d.k_blk0 = kblk; d.c_blk0 = cblk;
            d.n_k = V ? g.kmer_off[V] : 0; d.n_v = V;
            for (uint32_t v = 0; v < V; ++v) foff[vb + v] = fb + g.flank_off[v];
            kb += d.n_k; fb += V ? g.flank_off[V] : 0; vb += V;
            kblk += (uint32_t)(((uint64_t)d.n_k + KP_BLOCK - 1) / KP_BLOCK);
            cblk += (V + KP_ROWS - 1) / KP_ROWS;
        }
        foff[n_v] = fb;
        PlanDesc& end = p->desc[n_contigs];
        end.k_base = kb; end.v_base = vb; end.k_blk0 = kblk; end.c_blk0 = cblk;
    }
    const size_t isz = p->wide ? 8 : 4;
    unsigned long long* d_codes = nullptr;
    unsigned long long* d_ctr = nullptr;
    auto body = [&]() -> int {
        KK_TRY(hipEventCreate(&p->ev[0]));
        KK_TRY(hipEventCreate(&p->ev[1]));
        KK_TRY(hipMalloc(&p->d_kidx, std::max<uint64_t>(n_k, 1) * isz));
        KK_TRY(hipMalloc(&p->d_fidx, std::max<uint64_t>(n_f, 1) * isz));
        KK_TRY(hipMalloc((void**)&p->d_foff, foff.size() * sizeof(unsigned long long)));
        KK_TRY(hipMalloc((void**)&p->d_desc, p->desc.size() * sizeof(PlanDesc)));
        KK_TRY(hipHostMalloc((void**)&p->h_c, std::max<uint64_t>(n_v, 1) * 2, hipHostMallocDefault));
        p->device_bytes = (n_k + n_f) * isz + foff.size() * sizeof(unsigned long long) + p->desc.size() * sizeof(PlanDesc);
        uint64_t longest = 1;
        for (uint32_t c = 0; c < n_contigs; ++c) longest = std::max<uint64_t>(longest, std::max<uint64_t>(p->desc[c].n_k, foff[p->desc[c + 1].v_base] - foff[p->desc[c].v_base]));
        KK_TRY(hipMalloc((void**)&d_codes, std::min<uint64_t>(longest, kPlanChunk) * sizeof(unsigned long long)));
        KK_TRY(hipMalloc((void**)&d_ctr, 4 * sizeof(unsigned long long)));
        unsigned long long ctr[4] = {0ull, KK_EMPTY, 0ull, KK_EMPTY};
        KK_TRY(hipMemcpyAsync(d_ctr, ctr, sizeof ctr, hipMemcpyHostToDevice, counter->stream));
        KK_TRY(hipMemcpyAsync(p->d_foff, foff.data(), foff.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, counter->stream));
        KK_TRY(hipStreamSynchronize(counter->stream));
        for (uint32_t c = 0; c < n_contigs; ++c) {
            const PlanDesc& d = p->desc[c];
            if (int rc = plan_resolve(p, contigs[c].kmer_code, d.n_k, d.k_base, false, d_codes, d_ctr)) return rc;
            const uint64_t f0 = foff[d.v_base], f1 = foff[p->desc[c + 1].v_base];
            if (int rc = plan_resolve(p, contigs[c].flank_code, f1 - f0, f0, true, d_codes, d_ctr)) return rc;
        }
        KK_TRY(hipMemcpyAsync(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, counter->stream));
        KK_TRY(hipStreamSynchronize(counter->stream));
        p->unresolved = ctr[0] + ctr[2];
        if (p->unresolved && !p->lenient) {
            // the first one in index order: contig, then variant, then the variant's unique k-mers in front of its flanking ones
            uint32_t c[2] = {~0u, ~0u}, v[2] = {~0u, ~0u};
            uint64_t at[2] = {0, 0};
            if (ctr[0]) plan_locate<uint32_t>(p, contigs, false, ctr[1], &c[0], &v[0], &at[0]);
            if (ctr[2]) plan_locate<uint64_t>(p, contigs, true, ctr[3], &c[1], &v[1], &at[1]);
            const int w = (c[1] < c[0] || (c[1] == c[0] && v[1] < v[0])) ? 1 : 0;
            const uint64_t code = w ? contigs[c[w]].flank_code[contigs[c[w]].flank_off[v[w]] + at[w]] : contigs[c[w]].kmer_code[contigs[c[w]].kmer_off[v[w]] + at[w]];
            return fail(PG_ERR_INVALID, "pg_count_plan_new: contig %u, variant %u, %s k-mer %llu (code %llu) was not registered before the reads were counted (%llu such codes)",
                        c[w], v[w], w ? "flanking" : "unique", (unsigned long long)at[w], (unsigned long long)code, (unsigned long long)p->unresolved);
        }
        return PG_OK;
    };
    const int rc = body();
    if (d_codes) (void)hipFree(d_codes);
    if (d_ctr) (void)hipFree(d_ctr);
    if (rc != PG_OK) { pg_count_plan_destroy(p); return rc; }
    *out = p;
    return PG_OK;
}

int pg_count_plan_fill_host(pg_count_plan* p, uint64_t kmer_coverage, uint16_t* const* kmer_count, uint16_t* const* coverage) {
    if (!p) return fail(PG_ERR_INVALID, "pg_count_plan_fill_host: null plan");
    if (p->nc && (!kmer_count || !coverage)) return fail(PG_ERR_INVALID, "pg_count_plan_fill_host: null argument");
    for (uint32_t c = 0; c < p->nc; ++c)
        if ((p->desc[c].n_k && !kmer_count[c]) || (p->desc[c].n_v && !coverage[c])) return fail(PG_ERR_INVALID, "pg_count_plan_fill_host: contig %u has a null array", c);
    if (int rc = plan_use(p, "pg_count_plan_fill_host")) return rc;
    // (each of the three on its own: a call that failed half way leaves the rest to the next one)
    if (!p->d_out_k) { KK_TRY(hipMalloc((void**)&p->d_out_k, std::max<uint64_t>(p->n_k, 1) * 2)); p->device_bytes += p->n_k * 2; }
    if (!p->d_out_c) { KK_TRY(hipMalloc((void**)&p->d_out_c, std::max<uint64_t>(p->n_v, 1) * 2)); p->device_bytes += p->n_v * 2; }
    if (!p->h_k) KK_TRY(hipHostMalloc((void**)&p->h_k, std::max<uint64_t>(p->n_k, 1) * 2, hipHostMallocDefault));
    for (uint32_t c = 0; c < p->nc; ++c) {
        p->desc[c].out_k = p->d_out_k + p->desc[c].k_base;
        p->desc[c].out_c = p->d_out_c + p->desc[c].v_base;
    }
    if (int rc = plan_launch(p, kmer_coverage)) return rc;
    hipStream_t s = p->counter->stream;
    if (p->n_k) KK_TRY(hipMemcpyAsync(p->h_k, p->d_out_k, p->n_k * 2, hipMemcpyDeviceToHost, s));
    if (p->n_v) KK_TRY(hipMemcpyAsync(p->h_c, p->d_out_c, p->n_v * 2, hipMemcpyDeviceToHost, s));
    if (int rc = plan_finish(p)) return rc;
    for (uint32_t c = 0; c < p->nc; ++c) {
        const PlanDesc& d = p->desc[c];
        if (d.n_k) memcpy(kmer_count[c], p->h_k + d.k_base, (size_t)d.n_k * 2);
        if (d.n_v) memcpy(coverage[c], p->h_c + d.v_base, (size_t)d.n_v * 2);
    }
    return PG_OK;
}

int pg_count_plan_fill_device(pg_count_plan* p, uint64_t kmer_coverage, uint16_t* const* d_kmer_count, uint16_t* const* d_coverage) {
    if (!p) return fail(PG_ERR_INVALID, "pg_count_plan_fill_device: null plan");
    if (p->nc && (!d_kmer_count || !d_coverage)) return fail(PG_ERR_INVALID, "pg_count_plan_fill_device: null argument");
    for (uint32_t c = 0; c < p->nc; ++c)
        if ((p->desc[c].n_k && !d_kmer_count[c]) || (p->desc[c].n_v && !d_coverage[c])) return fail(PG_ERR_INVALID, "pg_count_plan_fill_device: contig %u has a null array", c);
    if (int rc = plan_use(p, "pg_count_plan_fill_device")) return rc;
    for (uint32_t c = 0; c < p->nc; ++c) {   // a host pointer would fault the kernel: refused here
        for (int which = 0; which < 2; ++which) {
            const void* ptr = which ? (const void*)d_coverage[c] : (const void*)d_kmer_count[c];
            if (!(which ? p->desc[c].n_v : p->desc[c].n_k)) continue;
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, ptr) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != p->counter->device) {
                (void)hipGetLastError();
                return fail(PG_ERR_INVALID, "pg_count_plan_fill_device: contig %u: the %s array is not in the memory of device %d", c, which ? "coverage" : "kmer_count", p->counter->device);
            }
        }
        p->desc[c].out_k = d_kmer_count[c];
        p->desc[c].out_c = d_coverage[c];
    }
    if (int rc = plan_launch(p, kmer_coverage)) return rc;
    return plan_finish(p);
}

int pg_count_plan_fill_job(pg_count_plan* p, uint64_t kmer_coverage, pg_job* job, uint32_t sample, char* err, size_t errlen) {
    auto said = [&](int rc) { if (rc != PG_OK && err && errlen) snprintf(err, errlen, "%s", g_err); return rc; };
    if (err && errlen) err[0] = 0;
    if (!p) return said(fail(PG_ERR_INVALID, "pg_count_plan_fill_job: null plan"));
    if (!job) return said(fail(PG_ERR_INVALID, "pg_count_plan_fill_job: null job"));
    if (int rc = plan_use(p, "pg_count_plan_fill_job")) return said(rc);
    std::vector<const uint32_t*> koff(p->nc);
    std::vector<uint16_t*> d_k(p->nc), d_c(p->nc);
    for (uint32_t c = 0; c < p->nc; ++c) koff[c] = p->koff[c].data();
    char text[400] = "";
    hipStream_t s = p->counter->stream;
    if (int rc = pgi_job_fill_begin(job, sample, p->counter->device, p->nc, p->n_variants.data(), koff.data(), (void*)s, d_k.data(), d_c.data(), text, sizeof text))
        return said(fail(rc, "pg_count_plan_fill_job: %s", text));
    for (uint32_t c = 0; c < p->nc; ++c) { p->desc[c].out_k = d_k[c]; p->desc[c].out_c = d_c[c]; }
    if (int rc = plan_launch(p, kmer_coverage)) return said(rc);
    std::vector<const uint16_t*> cov(p->nc);
    for (uint32_t c = 0; c < p->nc; ++c) {   // the job keeps a host copy of every chain's coverage: 2 bytes per variant come back
        const PlanDesc& d = p->desc[c];
        cov[c] = p->h_c + d.v_base;
        if (d.n_v) { const hipError_t e = hipMemcpyAsync(p->h_c + d.v_base, d_c[c], (size_t)d.n_v * 2, hipMemcpyDeviceToHost, s); if (e != hipSuccess) return said(hip_fail(e, "pg_count_plan_fill_job")); }
    }
    if (int rc = plan_finish(p)) return said(rc);
    if (int rc = pgi_job_fill_end(job, sample, p->nc, cov.data(), (void*)s, text, sizeof text)) return said(fail(rc, "pg_count_plan_fill_job: %s", text));
    return PG_OK;
}

int pg_count_plan_stats(const pg_count_plan* p, uint64_t* n_kmers, uint64_t* n_flanks, uint64_t* unresolved, uint64_t* device_bytes) {
    if (!p) return fail(PG_ERR_INVALID, "pg_count_plan_stats: null plan");
    if (n_kmers) *n_kmers = p->n_k;
    if (n_flanks) *n_flanks = p->n_f;
    if (unresolved) *unresolved = p->unresolved;
    if (device_bytes) *device_bytes = p->device_bytes;
    return PG_OK;
}

double pg_count_plan_last_fill_ms(const pg_count_plan* p) { return p ? p->last_ms : 0.0; }

}  // extern "C"
