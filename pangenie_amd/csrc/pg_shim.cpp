// pg_shim.cpp — C-ABI of include/pangenie_hmm.h on top of the HIP kernels (pg_kernels.hip): the probability table, jobs
// (their build, uploads and bin fetches), the coalescer of one-shot calls and the unit entry points of the emission /
// transition kernels.  A job's run schedule — pg_job_run — is pg_shim_run.cpp's; the output columns formed from a job's
// finished bins — calls, record calls, record GLs — are pg_shim_calls.cpp's; the three units share struct pg_job and the
// host's chain / index / plan types through pg_job.h.
//
// Host side of the boundary: argument checking, one device arena per job, H2D/D2H,
// launch order, hipEvent timing per kernel class.  No compute happens here except the
// ProbabilityTable, which the reference also builds on the host in long double before any
// HMM runs (reference src/commands.cpp:846, src/probabilitytable.cpp:28-45).
// There is NO CPU fallback: without a HIP device every entry point returns PG_ERR_DEVICE.
//
// A job = a set of CHAINS (one per (contig, path subset) — or per (sample, contig) in a cohort
// job) over a set of INDEX contigs.  Index arrays (positions, alleles, k-mer masks, path ->
// allele) are uploaded once per index contig; chains of a cohort job share them and own only
// their read counts, coverage, intermediates and results (reference src/commands.cpp:118-138:
// the index is sample-independent, update_readcount / set_coverage are the per-sample part).
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pangenie_hmm.h"
#include "pg_device.h"
#include "pg_job.h"
#include "pg_launch.h"

using namespace pgj;

// ---------------------------------------------------------------------------------------
//  ProbabilityTable (host, long double) — reference src/probabilitytable.cpp
// ---------------------------------------------------------------------------------------
struct pg_table {
    uint16_t cov_min = 0, cov_max = 0, count_max = 0;
    long double reg = 0.0L;
    std::vector<long double> p;  // [count][cov - cov_min][3], as the reference indexes it
    std::mutex mu;
};

namespace {

// reference src/probabilitytable.cpp:7-19
double error_param(double cov) {
    if (cov < 10.0) return 0.99;
    if (cov < 20) return 0.95;
    if (cov < 40) return 0.9;
    return 0.8;
}
// reference src/probabilitytable.cpp:75-81 (log(i): double overload; log(mean), exp: long double)
long double poisson_ld(long double mean, unsigned value) {
    long double sum = 0.0L;
    int v = (int)value;
    for (size_t i = 1; i <= value; ++i) sum += ::log((double)i);
    long double log_val = -mean + v * logl(mean) - sum;
    return expl(log_val);
}
// reference src/probabilitytable.cpp:83-85
long double geometric_ld(long double prob, unsigned value) { return powl(1.0L - prob, (long double)value) * prob; }

// reference src/probabilitytable.cpp:55-65 + src/copynumber.cpp:14-41
void compute_probability(const pg_table* t, uint16_t cov, uint16_t count, long double out[3]) {
    long double c0 = geometric_ld(error_param(cov), count);
    long double c1 = poisson_ld(cov / 2.0, count);
    long double c2 = poisson_ld(cov, count);
    if (t->reg > 0) {
        long double sum = c0 + c1 + c2 + 3.0L * t->reg;
        out[0] = (c0 + t->reg) / sum;
        out[1] = (c1 + t->reg) / sum;
        out[2] = 1.0L - out[0] - out[1];
    } else {
        out[0] = c0; out[1] = c1; out[2] = c2;
    }
}

bool in_table(const pg_table* t, uint16_t cov, uint16_t count) {
    return cov >= t->cov_min && cov < t->cov_max && count < t->count_max;
}

// (mantissa, exponent) view of the dense table, layout [cov][count][3].  Every job gets its OWN device
// copy inside its arena: a later pg_table_modify / pg_table_destroy cannot pull it away from under a
// resident job.
void table_snapshot(pg_table* t, std::vector<double>& m, std::vector<int32_t>& e, std::vector<unsigned char>& packed, DevTable* meta) {
    std::lock_guard<std::mutex> lock(t->mu);
    const uint32_t ncov = t->cov_max > t->cov_min ? t->cov_max - t->cov_min : 0;
    meta->cov_min = t->cov_min; meta->cov_max = t->cov_max; meta->count_max = t->count_max; meta->pad = 0;
    meta->reg = (double)t->reg;
    const size_t n = (size_t)ncov * t->count_max * 3;
    m.assign(n ? n : 1, 0.0);
    e.assign(n ? n : 1, 0);
    for (uint32_t c = 0; c < ncov; ++c)
        for (uint32_t k = 0; k < t->count_max; ++k)
            for (int i = 0; i < 3; ++i) {
                long double v = t->p[((size_t)k * ncov + c) * 3 + i];
                int ex = 0;
                long double mant = (v == 0.0L || v != v || isinf((double)v)) ? v : frexpl(v, &ex);
                m[((size_t)c * t->count_max + k) * 3 + i] = (double)mant;
                e[((size_t)c * t->count_max + k) * 3 + i] = ex;
            }
    // the same entries as 32-byte pieces {m0, m1, m2, int16 e0, e1, e2, 0} (DevTable::packed)
    packed.assign(n ? n / 3 * 32 : 32, 0);
    for (size_t q = 0; q < n / 3; ++q) {
        memcpy(&packed[q * 32], &m[q * 3], 24);
        for (int i = 0; i < 3; ++i) {
            const int32_t ex = e[q * 3 + i];
            const int16_t e16 = (int16_t)(ex < -32768 ? -32768 : (ex > 32767 ? 32767 : ex));   // (|exponent| <= 16445: long double's range)
            memcpy(&packed[q * 32 + 24 + 2 * i], &e16, 2);
        }
    }
}

}  // namespace

extern "C" pg_table* pg_table_create(uint16_t cov_min, uint16_t cov_max, uint16_t count_max, long double regularization) {
    pg_table* t = new pg_table();
    t->cov_min = cov_min; t->cov_max = cov_max; t->count_max = count_max; t->reg = regularization;
    const size_t ncov = cov_max > cov_min ? (size_t)(cov_max - cov_min) : 0;
    t->p.resize((size_t)count_max * ncov * 3);
    for (uint32_t i = 0; i < count_max; ++i)
        for (uint32_t j = 0; j < ncov; ++j)
            compute_probability(t, (uint16_t)(j + cov_min), (uint16_t)i, &t->p[((size_t)i * ncov + j) * 3]);
    return t;
}
extern "C" pg_table* pg_table_create_default(void) { return pg_table_create(0, 0, 0, 0.0L); }

extern "C" int pg_table_modify(pg_table* t, uint16_t cov, uint16_t count, long double p0, long double p1, long double p2) {
    if (!t || !in_table(t, cov, count)) return PG_ERR_INVALID;  // reference throws runtime_error here
    std::lock_guard<std::mutex> lock(t->mu);
    const size_t ncov = (size_t)(t->cov_max - t->cov_min);
    long double* e = &t->p[((size_t)count * ncov + (cov - t->cov_min)) * 3];
    e[0] = p0; e[1] = p1; e[2] = p2;
    return PG_OK;
}
extern "C" int pg_table_get(const pg_table* t, uint16_t cov, uint16_t count, long double out3[3]) {
    if (!t) return PG_ERR_INVALID;
    if (in_table(t, cov, count)) {
        const size_t ncov = (size_t)(t->cov_max - t->cov_min);
        const long double* e = &t->p[((size_t)count * ncov + (cov - t->cov_min)) * 3];
        out3[0] = e[0]; out3[1] = e[1]; out3[2] = e[2];
    } else {
        compute_probability(t, cov, count, out3);
    }
    return PG_OK;
}
extern "C" void pg_table_destroy(pg_table* t) { delete t; }

// ---------------------------------------------------------------------------------------
//  misc
// ---------------------------------------------------------------------------------------
extern "C" int pg_hmm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" const char* pg_hmm_version(void) { return "pangenie-hmm-mi355x 0.2 (gfx950, fp64)"; }

extern "C" int pg_hmm_geno_offsets(const pg_contig_batch* b, uint64_t* geno_off) {
    if (!b || !geno_off) return PG_ERR_INVALID;
    geno_off[0] = 0;
    for (uint32_t v = 0; v < b->n_variants; ++v) {
        const uint64_t A = b->allele_off[v + 1] - b->allele_off[v];
        geno_off[v + 1] = geno_off[v] + A * (A + 1) / 2;
    }
    return PG_OK;
}

// ---------------------------------------------------------------------------------------
//  jobs
// ---------------------------------------------------------------------------------------
static const char* const kKernelNames[PG_N_KERNEL_CLASSES] = {"k_prep", "k_compact", "k_records",
                                                              "k_sweep_phase1", "k_sweep_phase2", "k_bins"};

namespace {

// entries of posterior partials per column and slot pair (DevContig::T), the ONE place the arena plan and the chain
// descriptors take it from: threads per chain workgroup, half of them at HP = 32 (lanes l and l + 32 are folded: fold32)
uint32_t part_entries(const IndexHost& x) { return x.HP == 32u ? x.T / 2u : x.T; }

uint32_t pad_paths(uint32_t H) {
    for (uint32_t hp = 16; hp <= PG_MAX_PATHS; hp <<= 1)
        if (H <= hp) return hp;
    return 0;
}

int check_batch(const pg_contig_batch* b, bool need_counts, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return PG_ERR_INVALID; }
    const uint32_t V = b->n_variants;
    if (V > 0) {
        if (b->n_paths == 0) {  // reference src/columnindexer.cpp:18-22
            set_err(err, errlen, "HMM::index_columns: column 0 is not covered by any paths.");
            return PG_ERR_NO_PATHS;
        }
        if (!b->variant_pos || !b->kmer_off || !b->allele_off || !b->allele_id ||
            !b->allele_flags || !b->allele_kmer_off || !b->allele_kmer_mask || !b->path_allele || (need_counts && !b->coverage)) {
            set_err(err, errlen, "batch has null arrays");
            return PG_ERR_INVALID;
        }
        if (b->kmer_off[0] != 0 || b->allele_off[0] != 0) { set_err(err, errlen, "offset arrays must start at 0"); return PG_ERR_INVALID; }
        uint32_t maxA = 0;
        for (uint32_t v = 0; v < V; ++v) {
            if (b->kmer_off[v + 1] < b->kmer_off[v]) { set_err(err, errlen, "kmer_off is not monotonic at variant %u", v); return PG_ERR_INVALID; }
            if (b->allele_off[v + 1] <= b->allele_off[v]) {
                set_err(err, errlen, "variant %u has no alleles (allele_off must be strictly increasing)", v);
                return PG_ERR_INVALID;
            }
            const uint32_t A = b->allele_off[v + 1] - b->allele_off[v];
            if (A > maxA) maxA = A;
        }
        if (maxA > PG_MAX_ALLELES_PER_VARIANT) {
            set_err(err, errlen, "a variant has %u alleles; the device path supports at most %d per UniqueKmers object", maxA, PG_MAX_ALLELES_PER_VARIANT);
            return PG_ERR_UNSUPPORTED;
        }
        if (need_counts && b->kmer_off[V] > 0 && !b->kmer_count) { set_err(err, errlen, "kmer_count is null"); return PG_ERR_INVALID; }
    }
    if (b->n_paths > PG_MAX_PATHS) {
        set_err(err, errlen, "device path supports at most %d selected paths per chain (got %u); use path subsets (-a)", PG_MAX_PATHS, b->n_paths);
        return PG_ERR_UNSUPPORTED;
    }
    return PG_OK;
}

// Device arenas of finished one-shot jobs, kept for the next calls (the one-shot call creates and destroys a job per call,
// and a device allocation of tens of GB costs more than the job: the pages are mapped on first touch).  A POOL: the
// reference runs N constructors at a time on thread-pool workers (src/commands.cpp:949-978), so several arenas of
// different sizes are in use at once.  take(): the smallest cached arena of the device that is large enough.
// put(): keeps the arena unless the pool would then hold more than PG_ARENA_POOL_GB (default 200) — the smallest
// entries go first.  pg_hmm_release_cache() empties it; an allocation failure empties it and retries.
struct ArenaPool {
    struct Entry { int device; unsigned char* ptr; size_t bytes; };
    std::mutex mu;
    std::vector<Entry> free_list;
    // per device: PG_ARENA_POOL_GB, else 70 % of that device's memory (hipMemGetInfo; the caller has made `device` current)
    size_t limit(int device) {
        static const double env_gb = [] { const char* e = getenv("PG_ARENA_POOL_GB"); return e ? strtod(e, nullptr) : -1.0; }();
        if (env_gb >= 0.0) return (size_t)(env_gb * 1073741824.0);
        static size_t of_device[64] = {0};
        if (device < 0 || device >= 64) return (size_t)200 << 30;
        if (of_device[device] == 0) {
            size_t free_b = 0, total_b = 0;
            of_device[device] = (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) ? (size_t)(0.7 * (double)total_b) : ((size_t)200 << 30);
        }
        return of_device[device];
    }
    bool take(int device, size_t need, unsigned char** ptr, size_t* bytes) {
        std::lock_guard<std::mutex> lock(mu);
        int best = -1;
        for (size_t i = 0; i < free_list.size(); ++i)
            if (free_list[i].device == device && free_list[i].bytes >= need && (best < 0 || free_list[i].bytes < free_list[(size_t)best].bytes)) best = (int)i;
        if (best < 0) return false;
        *ptr = free_list[(size_t)best].ptr; *bytes = free_list[(size_t)best].bytes;
        free_list.erase(free_list.begin() + best);
        return true;
    }
    void put(int device, unsigned char* ptr, size_t bytes) {  // (the caller has made `device` current)
        std::vector<Entry> drop;
        {
            std::lock_guard<std::mutex> lock(mu);
            free_list.push_back({device, ptr, bytes});
            size_t total = 0;
            for (const Entry& e : free_list) if (e.device == device) total += e.bytes;
            const size_t lim = limit(device);
            while (total > lim) {   // (this device's smallest entries go first)
                long k = -1;
                for (size_t i = 0; i < free_list.size(); ++i)
                    if (free_list[i].device == device && (k < 0 || free_list[i].bytes < free_list[(size_t)k].bytes)) k = (long)i;
                if (k < 0) break;
                total -= free_list[(size_t)k].bytes;
                drop.push_back(free_list[(size_t)k]);
                free_list.erase(free_list.begin() + k);
            }
        }
        for (const Entry& e : drop)
            if (hipSetDevice(e.device) == hipSuccess) hipFree(e.ptr);
        if (!drop.empty()) hipSetDevice(device);
    }
    void clear() {
        std::vector<Entry> all;
        { std::lock_guard<std::mutex> lock(mu); all.swap(free_list); }
        for (const Entry& e : all)
            if (hipSetDevice(e.device) == hipSuccess) hipFree(e.ptr);
    }
} g_pool;

// Pinned staging buffers of the pipelined first run (upload_inputs: group B's copies).  Copies that are to run BESIDE a kernel
// must be on a stream that does not share its hardware queue with the kernel's (measured, profiles/r06_persist.txt: pageable
// copies on streams made for the purpose, and the same out of pinned memory, returned when group A's phase 1 ended, 122 - 135 ms
// later; on the job's second stream — the one the stream handshake vouches for — 17 ms), and a host thread can only feed such
// a stream asynchronously out of pinned memory.  So group B's host threads stage their sources through these themselves:
// 16 MB pieces, two per thread, kept for the life of the process.
struct PinnedPool {
    static constexpr size_t kBytes = (size_t)16 << 20;
    std::mutex mu;
    std::vector<unsigned char*> free_list;
    unsigned char* get() {
        { std::lock_guard<std::mutex> l(mu); if (!free_list.empty()) { unsigned char* p = free_list.back(); free_list.pop_back(); return p; } }
        void* p = nullptr;
        if (hipHostMalloc(&p, kBytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return (unsigned char*)p;
    }
    void put(unsigned char* p) { if (p) { std::lock_guard<std::mutex> l(mu); free_list.push_back(p); } }
    void clear() { std::lock_guard<std::mutex> l(mu); for (unsigned char* p : free_list) hipHostFree(p); free_list.clear(); }
} g_pinned;

}  // namespace

extern "C" void pg_job_destroy(pg_job* job) {
    if (!job) return;
    hipSetDevice(job->device);
    if (job->uploader.joinable()) job->uploader.join();
    for (auto& t : job->late_threads) if (t.joinable()) t.join();
    if (job->ev_late_made) { hipEventDestroy(job->ev_late[0]); hipEventDestroy(job->ev_late[1]); }
    if (job->copy_stream) { hipStreamSynchronize(job->copy_stream); hipStreamDestroy(job->copy_stream); }
    if (job->ev_fill) hipEventDestroy(job->ev_fill);
    if (job->calls_events) { hipEventDestroy(job->ev_calls[0]); hipEventDestroy(job->ev_calls[1]); }
    if (job->staging) hipHostFree(job->staging);
    if (job->alt_samples) hipFree(job->alt_samples);
    if (job->d_contigs_owned) hipFree(job->d_contigs_owned);
    if (job->stream) hipStreamSynchronize(job->stream);
    if (job->stream2) hipStreamSynchronize(job->stream2);
    job->calls.release();
    job->rcalls.release();
    job->rgl.release();
    job->rtext.release();
    job->rlines.release();
    job->rphase.release();
    job->ptext.release();
    job->plines.release();
    job->paneltext.release();
    job->panellines.release();
    job->combine.release();
    job->crec.release();
    job->rplans.clear();
    if (job->events) {
        for (auto& e : job->ev) hipEventDestroy(e);
        for (auto& e : job->ev_vit) hipEventDestroy(e);
        for (auto& e : job->ev_ix) hipEventDestroy(e);
    }
    if (job->events2)
        for (int q = 0; q < (int)PG_SCRATCH_BUFS; ++q) { hipEventDestroy(job->ev_sweep[q]); hipEventDestroy(job->ev_post[q]); }
    for (hipEvent_t e : job->ev_chunk) hipEventDestroy(e);
    for (hipEvent_t e : job->ev_piece) hipEventDestroy(e);
    if (job->ev_prep2) hipEventDestroy(job->ev_prep2);
    if (job->arena) {
        if (job->cache_arena) g_pool.put(job->device, job->arena, job->arena_bytes);
        else hipFree(job->arena);
    }
    if (job->stream2) hipStreamDestroy(job->stream2);
    if (job->stream) hipStreamDestroy(job->stream);
    delete job;
}

extern "C" void pg_hmm_release_cache(void) {
    int cur = -1;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    g_pool.clear();
    g_pinned.clear();
    if (have) hipSetDevice(cur);
}

namespace {

struct ChainSpec { uint32_t index; const uint16_t* kmer_count; const uint16_t* coverage; };

// The per-sample arrays of a COHORT job (host memory by contract, one pair of small arrays per chain: 8192 pageable copies
// for 4096 chains cost more than the kernels they feed) go through ONE pinned staging buffer laid out like the arena's
// sample run: `pieces` host threads pack a contiguous range of chains each and queue one large H2D copy for it.  The
// reference re-reads the counts per sample (src/commands.cpp:118-138); this is that step for a batch of samples.
// `dev_base` = device address of the sample run to fill; `cov_out[c]` takes the host copy of chain c's coverage.
int sample_upload(pg_job* job, const std::vector<ChainSpec>& specs, unsigned char* dev_base, hipStream_t stream,
                  std::vector<std::vector<uint16_t>>* cov_out, uint64_t* bytes, char* err, size_t errlen) {
    const size_t n = job->chains.size();
    if (!job->staging && !job->staging_refused) {
        hipError_t he = hipHostMalloc((void**)&job->staging, job->sample_bytes ? job->sample_bytes : 8, hipHostMallocDefault);
        if (he != hipSuccess) { (void)hipGetLastError(); job->staging = nullptr; job->staging_refused = true; }
    }
    if (!job->staging) {
        // The host would not pin sample_bytes (tens of GB for a large cohort): the chains' arrays go straight from the
        // caller's pageable buffers, one pair of copies per chain — slower (the runtime stages every copy), never a failure.
        const size_t lo0 = job->sample_lo;
        for (size_t c = 0; c < n; ++c) {
            ChainHost& ch = job->chains[c];
            const IndexHost& x = job->index[ch.index];
            if (x.V == 0) continue;
            HIP_TRY(hipMemcpyAsync(dev_base + (ch.o_cov - lo0), specs[c].coverage, (size_t)x.V * 2, hipMemcpyHostToDevice, stream));
            if (x.sumK) HIP_TRY(hipMemcpyAsync(dev_base + (ch.o_kcnt - lo0), specs[c].kmer_count, (size_t)x.sumK * 2, hipMemcpyHostToDevice, stream));
            if (bytes) *bytes += (uint64_t)x.V * 2 + (uint64_t)x.sumK * 2;
            if (cov_out) (*cov_out)[c].assign(specs[c].coverage, specs[c].coverage + x.V);
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return PG_OK;
    }
    size_t pieces = n / 64;   // (at most one copy per 64 chains)
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t cap = hw ? (hw > 32 ? 16 : (hw + 1) / 2) : 4;
    if (pieces > cap) pieces = cap;
    if (pieces < 1) pieces = 1;
    std::vector<int> rcs(pieces, (int)hipSuccess);
    std::vector<uint64_t> moved(pieces, 0);
    const size_t lo0 = job->sample_lo;
    auto work = [&](size_t k) {
        if (hipSetDevice(job->device) != hipSuccess) { rcs[k] = (int)hipErrorInvalidDevice; return; }
        const size_t c0 = n * k / pieces, c1 = n * (k + 1) / pieces;
        if (c0 >= c1) return;
        for (size_t c = c0; c < c1; ++c) {
            ChainHost& ch = job->chains[c];
            const IndexHost& x = job->index[ch.index];
            if (x.V == 0) continue;
            memcpy(job->staging + (ch.o_cov - lo0), specs[c].coverage, (size_t)x.V * 2);
            if (x.sumK) memcpy(job->staging + (ch.o_kcnt - lo0), specs[c].kmer_count, (size_t)x.sumK * 2);
            moved[k] += (uint64_t)x.V * 2 + (uint64_t)x.sumK * 2;
            if (cov_out) (*cov_out)[c].assign(specs[c].coverage, specs[c].coverage + x.V);
        }
        const size_t b0 = job->chains[c0].o_cov - lo0;
        const size_t b1 = c1 < n ? job->chains[c1].o_cov - lo0 : job->sample_bytes;
        if (b1 > b0) rcs[k] = (int)hipMemcpyAsync(dev_base + b0, job->staging + b0, b1 - b0, hipMemcpyHostToDevice, stream);
    };
    std::vector<std::thread> th;
    for (size_t k = 1; k < pieces; ++k) th.emplace_back(work, k);
    work(0);
    for (auto& t : th) t.join();
    for (size_t k = 0; k < pieces; ++k) {
        if (rcs[k] != (int)hipSuccess) { set_err(err, errlen, "sample upload: %s", hipGetErrorString((hipError_t)rcs[k])); return PG_ERR_DEVICE; }
        if (bytes) *bytes += moved[k];
    }
    HIP_TRY(hipStreamSynchronize(stream));   // (the staging buffer is free again, the set is complete)
    return PG_OK;
}

// H2D of the inputs into a planned job.  Copies are queued on the job's stream; pageable sources are
// staged by the runtime, so every call returns when its source has been read.
int upload_inputs(pg_job* job, const pg_contig_batch* batches, const std::vector<ChainSpec>& specs, bool with_index,
                  char* err, size_t errlen) {
    const double t0 = now_s();
    unsigned char* A = job->arena;
    hipStream_t s = job->stream;
    uint64_t bi = 0, bs = 0;
    // the copies are collected first: a large upload from pageable buffers (a whole genome through the one-shot call: 264
    // arrays, 1.06 GB) is then issued from several host threads on streams of their own — the runtime stages a pageable
    // source through its bounce buffers on the calling thread, one copy after the other: 24 ms on one thread
    struct Copy { void* dst; const void* src; size_t bytes; };
    // (the caller's arrays are valid until this call returns: once group B's threads run, an error return waits for them)
    struct LateGuard { pg_job* job; bool armed; ~LateGuard() { if (armed) join_late_threads(job); } } late_guard{job, false};
    std::vector<Copy> copies, late_copies;   // late: group B of a pipelined first run (pg_job::pipeline) — issued here, waited for in pg_job_run
    // (the pipelined first run needs the job's two streams to run side by side: asked once, here, where nothing is in flight)
    if (with_index && job->pipeline && !streams_concurrent(job, s)) job->pipeline = false;
    const bool pipe = with_index && job->pipeline;
    job->pipeline = false;   // (one upload: asked for again by whoever uploads and runs inside one call)
    std::vector<char> late(job->chains.size(), 0);
    if (pipe) for (size_t k = job->nA; k < job->grp_order.size(); ++k) late[job->grp_order[k]] = 1;
    bool cur_late = false;
#define UP(off, src, bytes, acc)                                                                              \
    do {                                                                                                      \
        if ((bytes) > 0) {                                                                                    \
            (cur_late ? late_copies : copies).push_back({(void*)(A + (off)), (const void*)(src), (size_t)(bytes)});  /* (host or device source) */ \
            acc += (uint64_t)(bytes);                                                                         \
        }                                                                                                     \
    } while (0)
    if (with_index) {
        record_plans_changed(job);   // (new allele ids: the record plans are checked against them again)
        for (size_t i = 0; i < job->index.size(); ++i) { job->rlines.drop_prefix(i); job->plines.drop_prefix(i); job->panellines.drop_prefix(i); }   // (a new index: its lines' fixed columns are the caller's to send again)
        job->prep_parts_ready = false;   // (a new column list: the extents of a preparation in parts are read again)
        for (size_t i = 0; i < job->index.size(); ++i) {
            const pg_contig_batch& b = batches[i];
            IndexHost& x = job->index[i];
            if (x.V == 0) continue;
            cur_late = pipe && late[i];   // (pipelined jobs: chain i over index contig i)
            UP(x.o_pos, b.variant_pos, (size_t)x.V * 8, bi);
            if (job->params.run_phasing) { x.pos.assign(b.variant_pos, b.variant_pos + x.V); job->vit_tq_ready = false; }
            UP(x.o_koff, b.kmer_off, ((size_t)x.V + 1) * 4, bi);
            UP(x.o_aoff, b.allele_off, ((size_t)x.V + 1) * 4, bi);
            UP(x.o_aid, b.allele_id, (size_t)x.sumA * 2, bi);
            UP(x.o_aflag, b.allele_flags, (size_t)x.sumA, bi);
            UP(x.o_akoff, b.allele_kmer_off, (size_t)x.sumA * 2, bi);
            UP(x.o_akmask, b.allele_kmer_mask, (size_t)x.sumA * 4, bi);
            UP(x.o_pa, b.path_allele, (size_t)x.V * x.H * 2, bi);
            UP(x.o_goff, x.goff.data(), ((size_t)x.V + 1) * 8, bi);
            if (x.wide_bytes) UP(x.o_widx, x.widx.data(), (size_t)x.V * 4, bi);
            if (x.aux_bytes) UP(x.o_auxidx, x.auxidx.data(), (size_t)x.V * 4, bi);
            UP(x.o_list_m4, x.list_m4.data(), x.list_m4.size() * 4, bi);
            UP(x.o_list_w, x.list_w.data(), x.list_w.size() * 4, bi);
            UP(x.o_list_b, x.list_b.data(), x.list_b.size() * 4, bi);
            UP(x.o_list_big, x.list_big.data(), x.list_big.size() * 4, bi);
        }
        cur_late = false;
        UP(job->o_tab_m, job->tab_m.data(), job->tab_m.size() * sizeof(double), bi);
        UP(job->o_tab_e, job->tab_e.data(), job->tab_e.size() * sizeof(int32_t), bi);
        UP(job->o_tab_p, job->tab_p.data(), job->tab_p.size(), bi);
    }
    if (job->cohort) {   // (host arrays by contract: packed into pinned staging, a few large copies)
        std::vector<std::vector<uint16_t>> cov(job->chains.size());
        const int rc = sample_upload(job, specs, job->cur_samples, s, &cov, &bs, err, errlen);
        if (rc != PG_OK) return rc;
        for (size_t c = 0; c < job->chains.size(); ++c) job->chains[c].coverage.swap(cov[c]);
    } else {
        const size_t rebase = (size_t)(job->cur_samples - (A + job->sample_lo));   // (0: jobs with device-resident counts never switch sets)
        for (size_t c = 0; c < job->chains.size(); ++c) {
            ChainHost& ch = job->chains[c];
            const IndexHost& x = job->index[ch.index];
            if (x.V == 0) continue;
            cur_late = pipe && late[c];
            UP(ch.o_cov + rebase, specs[c].coverage, (size_t)x.V * 2, bs);
            UP(ch.o_kcnt + rebase, specs[c].kmer_count, (size_t)x.sumK * 2, bs);
            ch.coverage.assign(specs[c].coverage, specs[c].coverage + x.V);
        }
    }
#undef UP
    // `list` split over up to four host threads (largest first onto the least loaded), each on a stream of its own; a thread
    // returns when its copies have been read AND have arrived
    auto shares_of = [](const std::vector<Copy>& list, unsigned nt) {
        std::vector<std::vector<Copy>> share(nt);
        std::vector<size_t> load(nt, 0), order(list.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return list[x].bytes > list[y].bytes; });
        for (size_t i : order) {
            unsigned best = 0;
            for (unsigned t = 1; t < nt; ++t) if (load[t] < load[best]) best = t;
            share[best].push_back(list[i]); load[best] += list[i].bytes;
        }
        return share;
    };
    const int device = job->device;
    auto copy_worker = [device](std::vector<Copy> mine, int* rc) {   // (by value: group B's threads outlive this call)
        hipStream_t st = nullptr;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        for (const Copy& c : mine) { if (e != hipSuccess) break; e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDefault, st); }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (st) hipStreamDestroy(st);
        *rc = (int)e;
    };
    {
        size_t total = 0;
        for (const Copy& c : copies) total += c.bytes;
        for (const Copy& c : late_copies) total += c.bytes;
        const unsigned nt = (total >= ((size_t)64 << 20) && copies.size() + late_copies.size() >= 8) ? 4u : 1u;
        if (nt > 1) {
            std::vector<std::vector<Copy>> share = shares_of(copies, nt);
            std::vector<int> rcs(nt, (int)hipSuccess);
            std::vector<std::thread> th;
            for (unsigned t = 1; t < nt; ++t) th.emplace_back(copy_worker, share[t], &rcs[t]);
            copy_worker(share[0], &rcs[0]);
            for (auto& t : th) t.join();
            for (unsigned t = 0; t < nt; ++t)
                if (rcs[t] != (int)hipSuccess) { set_err(err, errlen, "input upload: %s", hipGetErrorString((hipError_t)rcs[t])); return PG_ERR_DEVICE; }
        } else {
            for (const Copy& c : copies) HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDefault, s));
        }
        if (pipe) {
            // group B: on its way from here on; pg_job_run joins the threads when group A's kernels are running.  Staged through
            // pinned pieces by the thread itself (g_pinned: a pageable copy would wait for group A's kernels to end); a source
            // that is device memory is copied as it is.
            // All of them on the job's SECOND stream — the one stream known to run beside `s` (streams_concurrent): a stream made here
            // may share its hardware queue with `s`, and its copies then wait for group A's phase 1 to end (measured: 130 ms).
            hipStream_t st2 = job->stream2;
            auto staged_worker = [device, st2](std::vector<Copy> mine, int* rc) {
                hipStream_t st = st2;
                hipEvent_t ev[2] = {nullptr, nullptr};
                unsigned char* buf[2] = {g_pinned.get(), g_pinned.get()};
                hipError_t e = hipSetDevice(device);
                for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
                if (e == hipSuccess && (!buf[0] || !buf[1])) e = hipErrorOutOfMemory;
                size_t piece = 0;
                for (const Copy& c : mine) {
                    if (e != hipSuccess) break;
                    hipPointerAttribute_t at;
                    const bool on_device = hipPointerGetAttributes(&at, c.src) == hipSuccess && at.type == hipMemoryTypeDevice;
                    if (!on_device) (void)hipGetLastError();
                    if (on_device) { e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, st); continue; }
                    for (size_t off = 0; off < c.bytes && e == hipSuccess; off += PinnedPool::kBytes, ++piece) {
                        const size_t nby = std::min(PinnedPool::kBytes, c.bytes - off);
                        const int k = (int)(piece & 1u);
                        if (piece >= 2) e = hipEventSynchronize(ev[k]);   // (the piece two back has left this buffer)
                        if (e != hipSuccess) break;
                        memcpy(buf[k], (const unsigned char*)c.src + off, nby);
                        e = hipMemcpyAsync((unsigned char*)c.dst + off, buf[k], nby, hipMemcpyHostToDevice, st);
                        if (e == hipSuccess) e = hipEventRecord(ev[k], st);
                    }
                }
                // (the last pieces have left the pinned buffers before they go back to the pool; the stream itself is not waited for:
                //  group B's kernels are queued behind these copies, on the same stream)
                for (int k = 0; k < 2; ++k) if (ev[k] && piece > (size_t)k) { const hipError_t e2 = hipEventSynchronize(ev[k]); if (e == hipSuccess) e = e2; }
                for (int k = 0; k < 2; ++k) { if (ev[k]) hipEventDestroy(ev[k]); g_pinned.put(buf[k]); }
                *rc = (int)e;
            };
            const unsigned ntb = late_copies.size() >= 8 ? 4u : 1u;
            std::vector<std::vector<Copy>> share = shares_of(late_copies, ntb);
            job->late_rc.assign(ntb, (int)hipSuccess);
            job->late_threads.clear();
            for (unsigned t = 0; t < ntb; ++t) job->late_threads.emplace_back(staged_worker, share[t], &job->late_rc[t]);
            job->late_pending = true;
            late_guard.armed = true;
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (with_index) {
        // The index pass (pg_split.h): what the index alone decides — kept columns, present alleles, the column list; for split
        // chains the per-column index records — is formed NOW, once, for every chain over the index (reference: ColumnIndexer and
        // TransitionProbabilityComputer read positions and path alleles only, src/columnindexer.cpp:8-33,
        // src/transitionprobabilitycomputer.cpp:8-19).  A run of the job forms only what hangs on the sample's counts.
        HIP_TRY(hipEventRecord(job->ev_ix[0], s));
        HIP_TRY(hipMemsetAsync(job->ix_base, 0, job->ix_bytes, s));
        if (job->srec_bytes) HIP_TRY(hipMemsetAsync(job->srec_base, 0, job->srec_bytes, s));
        const uint32_t max_big = max_big_list(job);
        if (pipe) pgk_launch_index(job->d_reps_g, job->nA, job->max_v, max_big, 0, s);   // (group B's: pg_job_run, when its inputs have arrived)
        else pgk_launch_index(job->d_reps, (uint32_t)job->index.size(), job->max_v, max_big, job->any_split ? 1 : 0, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(job->ev_ix[1], s));
        HIP_TRY(hipStreamSynchronize(s));
        float ims = 0.f;
        HIP_TRY(hipEventElapsedTime(&ims, job->ev_ix[0], job->ev_ix[1]));
        job->index_ms = ims;
    }
    job->up_bytes[0] = bi; job->up_bytes[1] = bs;
    job->host_s[1] = now_s() - t0;
    late_guard.armed = false;   // (pg_job_run joins them, beside group A's kernels)
    return PG_OK;
}

// PG_KERNELS: the ONE override of the kernel choice — a comma-separated list of tokens that put a second implementation
// of a step beside the default one (cross-checks in tests/, measurements in tools/).  Nothing here is needed
// in production: the library takes every decision from the job (chain count, panel width, allele structure).
//   general | generic   no lean / lean-x / small kernels | the generic kernel for every HP >= 64
//   leanx | noleanx     k_sweep_leanx also in phase 1 of fused jobs | never
//   small | nosmall     k_sweep_small16 whatever the chain count | never
//   nolean2 notri nocls4 prepwave   phase 2 of triangle chains on the general kernel's ring | full columns | per-thread
//                       partials instead of class sums | k_prep for every object
//   fullcols            fused jobs at HP = 32 store and fetch whole 32 x 32 columns (DevContig::live = HP)
//   nosmall2            phase 2 of the 16-path chains of fused jobs on the general kernel (k_sweep_small16 for phase 1 only)
//   noleanx2            phase 2 of the 64-path triangle chains with multiallelic objects on the general kernel's triangle ring (per-thread
//                       partials) instead of k_sweep_leanx2 — cross-check
//   nowidef             a job with wide columns on 64-path chains of the general kernel runs chunked (as until round 6) instead of fused with
//                       those columns through their aux slots + k_bins_wide (DevContig::widef) — cross-check
//   persist             chunked jobs whose chains are all lean chains run phase 2 as the persistent pair k_sweep_lean<4> + k_post_loop
//                       (one launch each, chunks handed over on the device) instead of one launch per chunk (k_sweep_lean<3> + k_post).
//                       Opt-in: measured at par or behind on the whole-genome job (profiles/r06_persist.txt).  nopersist: the default, spelled out
//   nosparse            phase 1 of the lean chains of chunked jobs stores every column itself (no k_refill_lean) — cross-check
//   nosparse2           the chunk sweeps of phase 2 store every column into the scratch buffers although phase 1 is sparse (no second
//                       k_refill_lean per chunk; the sweeps wait for k_post to free a buffer) — cross-check
//   nopieces            phase 1 of a job whose chains are all sparse lean chains is one launch, and every chunk's partner columns are
//                       refilled in phase 2 (instead of a launch per piece with the refills of all pieces but the last beside phase 1)
//                       — cross-check
//   prepahead           a job that runs phase 1 in pieces prepares every variant ahead of phase 1 (instead of the ends of the chains ahead
//                       and their middle on the second stream beside the first pieces: pg_job::prep_beside) — cross-check
//   nosplit           the 16-path chains of fused jobs prepare every variant per sample (k_prep*, k_records, k_bins_lean2 / _x) instead of
//                       taking the split path (pg_split.h)
struct KernelChoice {
    bool general = false, generic = false, nolean2 = false, notri = false, nocls4 = false, prepwave = false, fullcols = false, nosmall2 = false, nosplit = false;
    bool persist = false, noleanx2 = false, nowidef = false, nosparse = false, nosparse2 = false, nopieces = false, prepahead = false;
    int leanx = -1, small = -1;   // -1: by the job, 0 / 1: forced
    std::string unknown;          // a token this list does not know
};
KernelChoice kernel_choice() {
    KernelChoice k;
    const char* e = getenv("PG_KERNELS");
    if (!e) return k;
    std::string tok;
    auto take = [&]() {
        if (tok == "general") k.general = true; else if (tok == "generic") k.generic = true;
        else if (tok == "leanx") k.leanx = 1; else if (tok == "noleanx") k.leanx = 0;
        else if (tok == "small") k.small = 1; else if (tok == "nosmall") k.small = 0;
        else if (tok == "nolean2") k.nolean2 = true; else if (tok == "notri") k.notri = true;
        else if (tok == "nocls4") k.nocls4 = true; else if (tok == "prepwave") k.prepwave = true;
        else if (tok == "fullcols") k.fullcols = true; else if (tok == "nosmall2") k.nosmall2 = true;
        else if (tok == "nosplit") k.nosplit = true;
        else if (tok == "noleanx2") k.noleanx2 = true;
        else if (tok == "nowidef") k.nowidef = true;
        else if (tok == "nosparse") k.nosparse = true;
        else if (tok == "nosparse2") k.nosparse2 = true;
        else if (tok == "nopieces") k.nopieces = true;
        else if (tok == "prepahead") k.prepahead = true;
        else if (tok == "persist") k.persist = true; else if (tok == "nopersist") k.persist = false;
        else if (!tok.empty()) k.unknown = tok;   // (a typo would quietly test the default path against itself: job creation fails)
        tok.clear();
    };
    for (const char* c = e; *c; ++c) { if (*c == ',' || *c == ' ') take(); else tok.push_back(*c); }
    take();
    return k;
}

// f(i) for every index contig: on worker threads when the contigs together hold enough variants to pay for them
template <class F>
void parallel_contigs(uint32_t n, const pg_contig_batch* batches, F&& f) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += batches[i].n_variants;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt ? (nt > 16 ? 16 : nt) : 4;
    if (nt > n) nt = n;
    if (n < 2 || total < 200000 || nt < 2) { for (uint32_t i = 0; i < n; ++i) f(i); return; }
    std::atomic<uint32_t> next{0};
    std::vector<std::thread> th;
    auto work = [&]() { for (uint32_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) f(i); };
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}

// ---------------------------------------------------------------------------------------
//  job_build: a job from the caller's arrays, as a sequence of steps — check, classify the index contigs, choose the mode
//  and every chain's kernels, lay the arena out, allocate it, fill and upload the descriptors, upload the inputs.
//  Deciding, laying out and touching the device are kept apart: a new kernel is a row of the tables below and a branch of
//  choose_chain_kernels.
// ---------------------------------------------------------------------------------------
// what the steps share: the caller's arguments and the kernel override, fixed for the whole construction
struct BuildArgs {
    uint32_t n_index;
    const pg_contig_batch* batches;
    const std::vector<ChainSpec>& specs;
    const pg_hmm_params& params;
    KernelChoice kc;
    bool cohort, cache_arena;
};

// destroys the job on every way out of job_build but the last
struct JobOwner {
    pg_job* job;
    ~JobOwner() { if (job) pg_job_destroy(job); }
    pg_job* release() { pg_job* j = job; job = nullptr; return j; }
};

int hip_fail(char* err, size_t errlen, const char* what, hipError_t e) {
    set_err(err, errlen, "%s: %s", what, hipGetErrorString(e));
    return PG_ERR_DEVICE;
}

int check_inputs(uint32_t n_index, const pg_contig_batch* batches, const std::vector<ChainSpec>& specs, const pg_table* table,
                 const pg_hmm_params* params, bool cohort, char* err, size_t errlen) {
    if (!batches || !table || !params || n_index == 0 || specs.empty()) { set_err(err, errlen, "null argument"); return PG_ERR_INVALID; }
    if (params->run_phasing) {
        // Viterbi (pg_viterbi.hip): a row of states is one wave's lanes, so at most 64 selected paths (the reference's
        // own callers pass at most 30, src/commands.cpp:939)
        for (const ChainSpec& sp : specs)
            if (batches[sp.index].n_paths > 64u) {
                set_err(err, errlen, "run_phasing: %u selected paths, the device Viterbi takes at most 64", batches[sp.index].n_paths);
                return PG_ERR_UNSUPPORTED;
            }
    }
    {   // (per-variant validation: contigs on worker threads when there is enough of it — a merged one-shot job of a whole
        //  genome spent 3 + 22 ms here and in the classification below, single-threaded, per round)
        std::vector<int> rcs(n_index, PG_OK);
        std::vector<std::string> msgs(n_index);
        parallel_contigs(n_index, batches, [&](uint32_t i) {
            char e[256] = {0};
            rcs[i] = check_batch(&batches[i], !cohort, e, sizeof(e));
            if (rcs[i] != PG_OK) msgs[i] = e;
        });
        for (uint32_t i = 0; i < n_index; ++i)
            if (rcs[i] != PG_OK) { set_err(err, errlen, "%s", msgs[i].c_str()); return rcs[i]; }
    }
    for (const ChainSpec& sp : specs) {
        const pg_contig_batch& b = batches[sp.index];
        if (b.n_variants > 0 && (!sp.coverage || (b.kmer_off[b.n_variants] > 0 && !sp.kmer_count))) {
            set_err(err, errlen, "a chain has null kmer_count / coverage arrays");
            return PG_ERR_INVALID;
        }
    }
    return PG_OK;
}

int select_device(int device, char* err, size_t errlen) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_err(err, errlen, "no HIP device available (no CPU fallback)"); return PG_ERR_DEVICE; }
    if (device < 0 || device >= ndev) { set_err(err, errlen, "bad device %d", device); return PG_ERR_INVALID; }
    if (hipSetDevice(device) != hipSuccess) { set_err(err, errlen, "hipSetDevice failed"); return PG_ERR_DEVICE; }
    return PG_OK;
}

// One index contig: its shape, the per-variant tables the kernels are handed (goff, n_kmers, the preparation lists, widx, auxidx)
// and which kernels its shape ALLOWS (lean, small, smallx, cls4, leanx, prep_fast, widef_cand) — what the job's mode makes of
// that is choose_job_mode's.  Host code only.  Two passes over the variants: the second, over those with more than two alleles,
// only when the first has found some that need a wide entry or an aux slot.  False: the wide-column tables exceed 64 GB.
bool classify_index_contig(const pg_contig_batch& b, const KernelChoice& kc, const pg_hmm_params& params, IndexHost& x) {
    const bool lean_ok = !kc.general && !kc.generic;
    x.V = b.n_variants; x.H = b.n_paths; x.HP = pad_paths(x.H ? x.H : 1);
    x.T = pgk_threads_for_hp(x.HP); x.RB = pg_rec_bytes(x.HP);
    x.sumK = x.V ? b.kmer_off[x.V] : 0; x.sumA = x.V ? b.allele_off[x.V] : 0;
    x.goff.assign((size_t)x.V + 1, 0);
    x.n_kmers.resize(x.V);
    if (x.V) { x.koff.assign(b.kmer_off, b.kmer_off + x.V + 1); x.aoff.assign(b.allele_off, b.allele_off + x.V + 1); }
    // k_prep_bi (four variants per wave) takes the two-allele objects with <= 32 k-mers of chains with <= 64 paths; the others
    // walk lists: list_m4 (3 .. PG_AMAX alleles, <= 64 k-mers: k_prep_m4), list_w (k_prep) and list_b (k_prep_bi's own).  Who wants
    // the lists is known after the pass only, so they start at the first object that is not k_prep_bi's — every one in front of
    // it is list_b's — and are dropped again below if nobody does.
    const bool fast_ok = x.H <= 64u && x.V > 0 && !kc.prepwave;
    const bool small_shape = lean_ok && x.HP == 16u && x.H == 16u;
    bool listing = false, two_alleles = true;
    uint64_t maxA = 1;
    uint32_t maxK = 0, n_bi = 0;
    for (uint32_t v = 0; v < x.V; ++v) {
        const uint64_t A = b.allele_off[v + 1] - b.allele_off[v];
        const uint32_t K = b.kmer_off[v + 1] - b.kmer_off[v];
        x.goff[v + 1] = x.goff[v] + A * (A + 1) / 2;
        x.n_kmers[v] = (uint16_t)K;
        if (A > maxA) maxA = A;
        if (K > maxK) maxK = K;
        if (A > 32u) x.list_big.push_back(v);
        if (A != 2) two_alleles = false;
        const bool bi = A == 2 && K <= 32u;
        if (bi) n_bi += 1;
        else if (!listing && (fast_ok || small_shape)) {
            listing = true;
            x.list_b.resize(v);
            for (uint32_t u = 0; u < v; ++u) x.list_b[u] = u;
        }
        if (listing) (bi ? x.list_b : (A >= 3 && A <= PG_AMAX && K <= 64u) ? x.list_m4 : x.list_w).push_back(v);
    }
    // prep_fast 1 = the whole chain is k_prep_bi's objects, 2 = at least half of it (k_prep takes the rest: HPRC-style panels and the
    // 15 + 1 sampled paths have a fifth of their objects multiallelic); PG_KERNELS=prepwave: k_prep for everything (cross-check)
    x.all_sb = two_alleles && maxK <= 32u;
    x.prep_fast = !fast_ok ? 0u : (x.all_sb ? 1u : (2u * n_bi >= x.V ? 2u : 0u));
    // (the same lists serve the split path's emission kernels — 16-path chains, whatever the share of biallelic objects)
    if (!(x.prep_fast == 2u || (small_shape && !x.all_sb))) {
        std::vector<uint32_t>().swap(x.list_b); std::vector<uint32_t>().swap(x.list_m4); std::vector<uint32_t>().swap(x.list_w);
    }
    x.n_lik = x.goff[x.V];
    x.pair_n = (uint32_t)(maxA < PG_AMAX ? maxA : PG_AMAX);
    x.part_slots = (x.pair_n + 1u) & ~1u;  // partials are stored as allele pairs (16-byte stores)
    if (x.part_slots < 2) x.part_slots = 2;
    x.lean = lean_ok && x.HP == 64 && x.H == 64 && maxA == 2 && x.V > 0;
    x.small = small_shape && maxA == 2 && x.V > 0;   // (and enough of them: choose_job_mode)
    // the same shape with multiallelic objects — 15 sampled paths + the reference path, bubbles keeping every allele those
    // paths carry (src/commands.cpp:799-803, src/multiallelicuniquekmers.cpp:195-232): k_sweep_small16x, any allele count
    // per object (narrow columns from the record's table, wide ones from the side table: per COLUMN)
    x.smallx = small_shape && maxA > 2 && x.V > 0;
    // PG_KERNELS=nocls4: per-thread partials + k_bins (cross-check)
    // (the class sums are formed by a half-chain's ONE compute wave: 16 paths, and 32 when the kernel is built with 16 rows per lane)
    x.cls4 = (x.HP == 16 || (x.HP == 32 && pgk_threads_for_hp(32) == 64u)) && x.H == x.HP && maxA == 2 && x.V > 0 && !kc.nocls4;
    // PG_KERNELS=noleanx: the general kernel (cross-check)
    x.leanx = lean_ok && (x.HP == 128 || x.HP == 64) && !x.lean && maxA >= 1 && maxA <= PG_AMAX && x.V > 0 && kc.leanx != 0;
    // Variants with more than PG_AMAX alleles may turn into WIDE columns (as many distinct alleles on the selected paths): a wide
    // entry with room for min(A, H) local alleles each.  Aux slots, where a fused phase 2 leaves what k_bins_x / k_bins_wide
    // finish: smallx chains — a variant with 3 .. PG_AMAX alleles as its (up to) fifteen bins (128 bytes), one with more as a whole
    // column (or as bins, if its paths carry at most PG_AMAX of them); 64-path chains of the general kernel (DevContig::widef) —
    // one column (8 HP^2 bytes) for every variant that may turn into a wide column.
    const bool wide = maxA > PG_AMAX;
    const bool widef_shape = x.HP == 64 && wide && x.V > 0 && !kc.nowidef && !kc.generic && params.run_genotyping && !params.run_phasing;
    if (wide || x.smallx) {
        const bool aux_x = x.smallx;
        const uint64_t bins_slot = 128u /* fifteen bins */, col_slot = (uint64_t)x.HP * x.HP * 8u;
        uint64_t woff = 0, ao = 0;
        if (wide) x.widx.assign(x.V, PG_WIDE_NONE);
        if (aux_x || widef_shape) x.auxidx.assign(x.V, PG_WIDE_NONE);
        for (uint32_t v = 0; v < x.V; ++v) {
            const uint64_t A = b.allele_off[v + 1] - b.allele_off[v];
            if (A <= 2) continue;
            const bool cand = A > PG_AMAX;
            if (cand) {
                uint64_t nl = A < x.H ? A : x.H;
                if (nl > PG_WIDE_MAX) nl = PG_WIDE_MAX;
                x.widx[v] = (uint32_t)(woff / 16);
                woff += pg_wide_entry_bytes((uint32_t)nl);
                if (woff / 16 >= 0xFFFFFFF0ull) return false;
            }
            if (!aux_x && !(widef_shape && cand)) continue;
            x.auxidx[v] = (uint32_t)(ao / 16);
            if (cand) x.n_wide_cand += 1;
            ao += !cand ? bins_slot : (aux_x && bins_slot > col_slot) ? bins_slot : col_slot;
        }
        if (wide) x.wide_bytes = woff;
        const bool fits = ao / 16 < 0xFFFFFFF0ull;
        if (aux_x) { if (fits) x.aux_bytes = ao; else x.smallx = false; }   // (the general kernel then)
        if (widef_shape) {
            if (fits) { x.aux_bytes = ao; x.widef_cand = true; }
            else { x.auxidx.clear(); x.n_wide_cand = 0; }
        }
    }
    return true;
}

int classify_index(pg_job* job, const BuildArgs& a, char* err, size_t errlen) {
    job->index.resize(a.n_index);
    std::vector<char> ok(a.n_index, 1);
    parallel_contigs(a.n_index, a.batches, [&](uint32_t i) { ok[i] = classify_index_contig(a.batches[i], a.kc, a.params, job->index[i]); });
    for (uint32_t i = 0; i < a.n_index; ++i) {
        if (!ok[i]) { set_err(err, errlen, "wide-column tables exceed 64 GB"); return PG_ERR_UNSUPPORTED; }
        job->max_v = std::max(job->max_v, job->index[i].V);
    }
    return PG_OK;
}

// The job's mode, decided from the classified contigs: which of the kernels a contig's shape allows its chains get (the small
// kernels' crossover), fused or chunked, the chunk size, the persistent pair, the split path.  chunk_cap: 0, or the most chunk
// columns this attempt may plan for (job_build's retry of a chunked job whose arena did not fit).  No device objects are made.
void choose_job_mode(pg_job* job, const BuildArgs& a, size_t chunk_cap) {
    const KernelChoice& kc = a.kc;
    const pg_hmm_params& params = a.params;
    const uint32_t n_chains = (uint32_t)a.specs.size();
    job->persist = false; job->post_blocks = 0; job->any_split = false; job->sparse = false; job->sparse2 = false; job->piece_chunks = 0; job->n_pieces = 1;
    {
        // k_sweep_small16 packs four H = 16 half-chains into a wave: a throughput kernel.  A single chain is faster on the
        // general kernel (four states per lane instead of sixteen: 375 vs 470 ns per column); PG_KERNELS=small / nosmall forces.
        // Where the whole STEP crosses over (round 6, tools/exp_small_crossover.py, profiles/r06_small_crossover.txt: 8 contigs x
        // 8000 variants per sample, fused; with the small kernels comes the split path, 0.6 against 2.5 ms of per-variant work at
        // 512 chains) — step ms, small kernels / general kernel:
        //   chains        64           128          256          512           1024
        //   biallelic     5.99 / 5.39  6.13 / 5.82  6.33 / 7.35  6.98 / 9.28   9.16 / 14.01
        //   a fifth 3-5   8.15 / 5.32  8.39 / 6.15  8.71 / 8.33  9.30 / 12.01  11.81 / 19.48
        // -> from 256 chains on when every such chain is biallelic, from 320 when some have multiallelic objects (512 for both
        //    until round 6: a 256-chain biallelic cohort ran 14 % below what it could).
        size_t n_small_chains = 0, n_x_chains = 0;
        for (const ChainSpec& sp : a.specs) {
            n_small_chains += (job->index[sp.index].small || job->index[sp.index].smallx) ? 1 : 0;
            n_x_chains += job->index[sp.index].smallx ? 1 : 0;
        }
        const bool use = kc.small >= 0 ? kc.small == 1 : n_small_chains >= (n_x_chains ? 320u : 256u);
        if (!use) for (auto& x : job->index) { x.small = false; x.smallx = false; if (!x.widef_cand) x.aux_bytes = 0; }
    }
    // A WIDE column (more than PG_AMAX alleles on the selected paths) costs that column, not the job, on the kernels that
    // take it inside a fused phase 2 — k_sweep_small16x (its column goes to the aux slot, k_bins_wide forms the bins); a
    // chain of any other kernel with such an object still makes the job chunked (k_post is their only wide path)
    bool wide_candidates = false, generic_needed = false;
    for (const IndexHost& x : job->index) {
        // (a k_sweep_small16x chain left with ONE column that is wide has its bins formed by k_bins_wide_s — the split path; jobs
        //  that cannot take the split path — run_phasing, 2^32 bins — go chunked as before round 5 instead of failing such a chain
        //  with PG_DEVERR_WIDE_FUSED at run time.  PG_KERNELS=nosplit keeps the fused job: a cross-check switch.)
        const bool split_possible = kc.nosplit || (!params.run_phasing && params.run_genotyping && x.n_lik < 0xFFFFFFF0ull);
        if (x.wide_bytes && !(x.smallx && !kc.nosmall2 && split_possible) && !x.widef_cand) wide_candidates = true;
        if (x.HP >= 256) generic_needed = true;
    }
    // ---- sweep mode ------------------------------------------------------------------------
    size_t per_col = 0;  // scratch bytes per chunk column over all chains (PG_SCRATCH_BUFS buffers x 2 roles)
    for (const ChainSpec& sp : a.specs) { const IndexHost& x = job->index[sp.index]; per_col += (size_t)2 * PG_SCRATCH_BUFS * x.HP * x.HP * sizeof(double); }
    // wide columns of chains that are not k_sweep_small16x's (wide_candidates, above) and HP >= 256 have their posteriors formed by k_post only: such jobs always run chunked
    bool want = n_chains * 2u < 128u;  // fewer workgroups than half the CUs
    // merged one-shot calls (cache_arena): always the mode — and with it the kernels — every one of them runs alone, so
    // that a caller's result does not depend on who else happened to be in flight (bit for bit, by construction)
    if (a.cache_arena) want = true;
    if (const char* m = getenv("PG_SWEEP_MODE")) {
        if (!strcmp(m, "fused")) want = false;
        else if (!strcmp(m, "chunked")) want = true;
    }
    if (wide_candidates || generic_needed || kc.generic) want = true;
    job->chunked = want && job->max_v > 0 && params.run_genotyping;
    if (job->chunked) for (auto& x : job->index) { x.cls4 = false; x.aux_bytes = 0; }   // (chunked jobs form their posteriors in k_post)
    if (kc.nosmall2) for (auto& x : job->index) if (!x.widef_cand) x.aux_bytes = 0;
    for (auto& x : job->index) x.widef = x.widef_cand && !job->chunked && x.aux_bytes != 0;
    // k_sweep_leanx is a latency kernel (lone chains: 1470 vs 2645 ns per column at 128 paths); phase 1 of a fused job
    // with hundreds of chains is bound by HBM writes, where the general kernel measured faster (7.8 vs 8.9 ms on 128 chains
    // of 128 paths).  PG_KERNELS=leanx forces it there too.
    if (!job->chunked && kc.leanx != 1) for (auto& x : job->index) x.leanx = false;
    if (job->chunked) {
        // 8192 columns per chunk (round 6; 4096 before): 25 chunk rounds instead of 50 on the whole genome.  With k_post no longer
        // the bound (post_lean64, the idle CUs shared out over the chains still running) what a chunk round costs beyond its columns
        // is its launches and resume prologues, and how much THAT is varies from box to box: 4096 / 6144 / 8192 / 12288 columns:
        // 128.7 / 128.5 / 126.9 / - ms of phase 2 on one box, 133.8 / 127.8 / 127.9 / 127.5 on another (profiles/r06_persist.txt 8).
        size_t k = 8192;
        const size_t budget = (size_t)39 << 30;   // (three buffers: 8192 columns for the 24 chains of a whole genome at 64 paths)
        if (per_col * k > budget) k = budget / per_col;
        if (const char* e = getenv("PG_CHUNK_COLS")) { const long v = strtol(e, nullptr, 0); if (v > 0) k = (size_t)v; }
        if (chunk_cap && k > chunk_cap) k = chunk_cap;
        const size_t half = (size_t)job->max_v / 2 + 1;
        if (k > half) k = half;
        if (k < 1) k = 1;
        job->chunk_cols = (uint32_t)k;
        job->n_chunks = (uint32_t)((half + k - 1) / k);
        // the persistent phase 2: every chain a lean chain (or empty), an even chunk (the lean step runs two columns per loop
        // iteration) unless a chunk is the whole half, and a CU for every workgroup of the two kernels that wait for each other
        bool all_lean = kc.persist, any_lean = false;
        for (const ChainSpec& sp : a.specs) { const IndexHost& x = job->index[sp.index]; if (x.V && !x.lean) all_lean = false; if (x.lean) any_lean = true; }
        if (all_lean && any_lean && ((job->chunk_cols & 1u) == 0u || job->n_chunks == 1u)) {
            uint32_t cus = 0;
            uint32_t pb = pgk_post_blocks(n_chains, job->chunk_cols, &cus);
            // (the sweep's workgroups MUST all be running — a k_post_loop block that is not merely takes no work —: eight CUs are
            //  left free beside the two grids, whatever else may hold a CU)
            const uint32_t margin = 8u;
            if (n_chains <= 64u && cus > 2u * n_chains + margin) {   // (k_post_loop looks at all chains with one lane each)
                const uint32_t room = (cus - 2u * n_chains - margin) / n_chains;
                if (pb > room) pb = room;
                if (const char* e = getenv("PG_POST_BLOCKS")) { const long v = strtol(e, nullptr, 0); if (v >= 1 && (uint32_t)v < pb) pb = (uint32_t)v; }   // (experiments: fewer)
                if (pb >= 1u) { job->persist = true; job->post_blocks = pb; }
            }
        }
        // the sparse phase 1 of lean chains: whole refill segments per chunk, and CUs beside the chains for k_refill_lean (what
        // pgk_launch_post asks before it shares the idle CUs out)
        if (any_lean && !job->persist && !kc.nosparse && job->chunk_cols % PG_LEAN_SPARSE == 0u) {
            uint32_t cus = 0;
            (void)pgk_post_blocks(n_chains, job->chunk_cols, &cus);
            job->sparse = cus >= 2u * n_chains + n_chains;
            // the sparse phase 2: the scratch buffers are the second stream's alone only if no chain's chunk sweep writes them
            bool only_lean = true;
            for (const ChainSpec& sp : a.specs) { const IndexHost& x = job->index[sp.index]; if (x.V && !x.lean) only_lean = false; }
            job->sparse2 = job->sparse && only_lean && !kc.nosparse2;
            // phase 1 in pieces of PG_PIECE_CHUNKS partner chunks each (see pg_job::n_pieces)
            if (job->sparse2 && !kc.nopieces) {
                uint32_t G = PG_PIECE_CHUNKS_DEFAULT;
                if (const char* e = getenv("PG_PIECE_CHUNKS")) { const long v = strtol(e, nullptr, 0); if (v >= 1 && v <= 0xFFFF) G = (uint32_t)v; }
                // (the piece and G travel in the 16-bit halves of the kernel's `chunk` argument)
                if ((unsigned long long)G * job->chunk_cols <= 0xFFFFFFFFull && (job->n_chunks + G - 1u) / G <= 0x10000u) {
                    job->piece_chunks = G;
                    job->n_pieces = (job->n_chunks + G - 1u) / G;
                    // the refills beside phase 1 have a whole piece's time for a fraction of its columns: on a third of the idle CUs they
                    // still end before the next piece does, and slow the chains beside them less than at full width (genome24_h64, phase 1:
                    // + 3.7 ms on all idle CUs, + 0.3 .. 1.0 ms on a half or a quarter; on an eighth they no longer end in time —
                    // profiles/r11_refill_beside_phase1.txt).  PG_PIECE_REFILL_BLOCKS: experiments
                    job->piece_refill_blocks = std::max<uint32_t>((cus - 2u * n_chains) / 3u, 1u);
                    if (const char* e = getenv("PG_PIECE_REFILL_BLOCKS")) { const long v = strtol(e, nullptr, 0); if (v >= 1 && v <= 0xFFFF) job->piece_refill_blocks = (uint32_t)v; }
                }
            }
        }
    }
    // ---- the split path: which index contigs' chains take it (pg_device.h) ---------------------------
    for (auto& x : job->index) {
        const bool s1 = x.small && !job->chunked && x.cls4 && !kc.nosmall2;   // (DevContig::small == 2)
        const bool s2 = x.smallx && !job->chunked && !kc.nosmall2;            // (DevContig::smallx == 2)
        const bool ok = !kc.nosplit && !params.run_phasing && params.run_genotyping && x.n_lik < 0xFFFFFFF0ull && x.V > 0;
        x.split = !ok ? 0u : (s1 ? 1u : (s2 ? 2u : 0u));
        if (x.split) job->any_split = true;
    }
}

// ---- which kernels run a chain -------------------------------------------------------------
// A kernel's identity; its row of the table gives its launch bits (pg_launch.h) and its name in the plan text (pg_job_plan):
// the launch masks and the text are both made from a chain's ChainKernels and from nothing else.
enum SweepKernel : uint8_t {
    SW_NONE, SW_HP16, SW_HP32, SW_HP64, SW_HP128, SW_GENERIC, SW_GENERIC64, SW_LEAN, SW_LEAN_TRI, SW_LEAN2, SW_LEANX128, SW_LEANX64,
    SW_TRI1, SW_LEANX_TRI, SW_LEANX_TRIW, SW_LEANX2, SW_SMALL16, SW_SMALL16X, SW_COUNT
};
// (phased: the phase is a template argument, "<1>" .. "<4>" in the text.  PG_SWEEP_TRI goes with every kernel that stores
//  triangles: the launcher reads it beside PG_SWEEP_LEAN only.  The four-half-chains-per-wave kernels have no bit: they walk
//  chain-id lists, pgk_launch_sweep_small / _smallx.)
struct SweepRow { uint32_t bits; const char* name; bool phased; };
const SweepRow kSweep[SW_COUNT] = {
    {0u, "", false},
    {PG_SWEEP_HP16, "k_sweep<16,4>", true}, {PG_SWEEP_HP32, "k_sweep<32,8>", true},
    {PG_SWEEP_HP64, "k_sweep<64,16>", true}, {PG_SWEEP_HP128, "k_sweep<128,32>", true},
    {PG_SWEEP_GENERIC, "k_sweep_generic", true},
    {PG_SWEEP_GENERIC64 | PG_SWEEP_GENERIC /* one generic launch covers both */, "k_sweep_generic", true},
    {PG_SWEEP_LEAN, "k_sweep_lean", true}, {PG_SWEEP_LEAN | PG_SWEEP_TRI, "k_sweep_lean_tri", true}, {PG_SWEEP_LEAN2, "k_sweep_lean2", false},
    {PG_SWEEP_LEANX128, "k_sweep_leanx", true}, {PG_SWEEP_LEANX64, "k_sweep_leanx", true},
    {PG_SWEEP_TRI1 | PG_SWEEP_TRI, "k_sweep_tri1", false}, {PG_SWEEP_LEANX_TRI | PG_SWEEP_TRI, "k_sweep_leanx_tri", false},
    {PG_SWEEP_LEANX_TRIW | PG_SWEEP_TRI, "k_sweep_leanx_triw", false}, {PG_SWEEP_LEANX2, "k_sweep_leanx2", false},
    {0u, "k_sweep_small16", true}, {0u, "k_sweep_small16x", true}
};
enum BinsKernel : uint8_t { BN_NONE, BN_FULL, BN_LEAN2, BN_THIN, BN_X, BN_WIDE, BN_S, BN_WIDE_S, BN_Q, BN_COUNT };
struct BinsRow { uint32_t bit; const char* name; };
const BinsRow kBins[BN_COUNT] = {{0u, ""}, {PG_BINS_FULL, "k_bins"}, {PG_BINS_LEAN2, "k_bins_lean2"}, {PG_BINS_THIN, "k_bins_thin"}, {PG_BINS_X, "k_bins_x"},
                                 {PG_BINS_WIDE, "k_bins_wide"}, {PG_BINS_S, "k_bins_s"}, {PG_BINS_WIDE_S, "k_bins_wide_s"}, {PG_BINS_Q, "k_bins_q"}};
enum PrepKernels : uint8_t { PREP_S_BI, PREP_S_LISTS, PREP_BI, PREP_BI_LISTS, PREP_W, PREP_COUNT };
const char* const kPrepName[PREP_COUNT] = {
    "index pass once (k_index_scan, k_compact, k_index_cols); per run k_prep_s_bi",
    "index pass once (k_index_scan, k_compact, k_index_cols); per run k_prep_s_bi + k_prep_s_m4 + k_prep_s_w",
    "index pass once (k_index_scan, k_compact); per run k_prep_bi + k_records",
    "index pass once (k_index_scan, k_compact); per run k_prep_bi + k_prep_m4 + k_prep + k_records",
    "index pass once (k_index_scan, k_compact); per run k_prep + k_records"
};
enum PostKernels : uint8_t { POST_NONE, POST_CHUNKS, POST_LOOP };   // fused: bins | k_post per chunk | the persistent pair's k_post_loop

struct ChainKernels {
    PrepKernels prep = PREP_W;
    SweepKernel phase1 = SW_NONE;
    SweepKernel phase2 = SW_NONE;    // fused jobs: the posterior half; chunked jobs: the store-only kernel of every chunk
    // the general (or generic) kernel whose launches walk this chain too, SW_NONE: none does.  It does a phase that has no kernel
    // of its own and returns at once in the others
    SweepKernel general = SW_NONE;
    PostKernels post = POST_NONE;
    BinsKernel bins = BN_NONE;       // who forms the chain's bins in a fused job ...
    BinsKernel bins_one = BN_NONE;   // ... those of a k_sweep_small16x chain left with a single column
    BinsKernel bins_wide = BN_NONE;  // ... and those of its wide columns
    // the values of the DevContig fields of the same names
    uint32_t lean = 0, leanx = 0, leanx2 = 0, tri = 0, cls4 = 0, small = 0, smallx = 0, widef = 0, T = 0, sparse = 0, sparse2 = 0;
};

// Every chain's kernels from its index contig's class and the job's mode; from them the two launch masks.
std::vector<ChainKernels> choose_chain_kernels(pg_job* job, const BuildArgs& a) {
    const KernelChoice& kc = a.kc;
    const bool fused = !job->chunked;
    std::vector<ChainKernels> kernels(a.specs.size());
    job->hp_mask = 0; job->bins_which = 0; job->vit_bits = 0;
    for (size_t c = 0; c < kernels.size(); ++c) {
        const IndexHost& x = job->index[a.specs[c].index];
        ChainKernels& k = kernels[c];
        // fused jobs: lean chains store / read their columns as compact upper triangles (18 KB instead of 32 KB per
        // column: half the sweep's HBM bytes and of the arena); PG_KERNELS=notri keeps full columns (cross-check)
        // (round 6: and the 64-path chains with multiallelic objects — every column narrow — whose phase 1 runs on the general
        //  kernel: it stores the same triangles, phase 2 reads them through its triangle ring: DevContig::tri == 1)
        // (DevContig::widef chains too: their wide columns leave phase 2 through aux slots, k_bins_wide reads the stored triangle)
        const bool tri_multi = !x.lean && !x.leanx && x.HP == 64 && x.H == 64 && (!x.wide_bytes || x.widef) && x.pair_n > 2 && !kc.generic && !kc.general;
        const bool tri = (x.lean || tri_multi) && fused && !kc.notri;
        k.lean = x.lean ? 1u : 0u; k.cls4 = x.cls4 ? 1u : 0u; k.widef = x.widef ? 1u : 0u; k.T = part_entries(x);
        k.small = x.small ? ((fused && x.cls4 && !kc.nosmall2) ? 2u : 1u) : 0u;   // 2: phase 2 on k_sweep_small16 too (class sums)
        k.smallx = x.smallx ? ((fused && !kc.nosmall2) ? 2u : 1u) : 0u;
        k.tri = tri ? ((kc.nolean2 || !x.lean) ? 1u : 2u) : 0u;   // (PG_KERNELS=nolean2, and chains with multiallelic objects: phase 2 of triangle chains on the general kernel's triangle ring)
        if (k.tri == 1u && !x.lean && x.HP == 64u && !kc.noleanx2 && !a.params.run_phasing && !x.widef) { k.leanx2 = 1u; k.T = 64u; }   // phase 2 on k_sweep_leanx2 (no wide columns there)
        // phase 1 of the triangle chains that are not lean chains: the lean-x step with triangle stores (DevContig::leanx == 2; it
        // needs the column-order records of the general kernel, which phase 2 reads too) — PG_KERNELS=noleanx: the general kernel
        // with triangle stores (k_sweep_tri1)
        k.leanx = (k.tri && !x.lean && kc.leanx != 0) ? 2u : (x.leanx ? 1u : 0u);
        k.sparse = (job->sparse && k.lean == 1u && k.tri == 0u) ? 1u : 0u;   // (chunked jobs have no triangle chains)
        k.sparse2 = (job->sparse2 && k.sparse) ? 1u : 0u;
        k.prep = x.split ? (x.all_sb ? PREP_S_BI : PREP_S_LISTS) : x.prep_fast == 1u ? PREP_BI : x.prep_fast == 2u ? PREP_BI_LISTS : PREP_W;

        const SweepKernel own = x.HP >= 256 ? SW_GENERIC : (kc.generic && x.HP >= 64) ? SW_GENERIC64
                              : x.HP == 16 ? SW_HP16 : x.HP == 32 ? SW_HP32 : x.HP == 64 ? SW_HP64 : SW_HP128;
        const SweepKernel leanx_kernel = x.HP == 128 ? SW_LEANX128 : SW_LEANX64;
        // (split chains never run on the general kernel; nor do, in a chunked job — no phase 2 —, the chains whose store-only phases
        //  have a kernel of their own: the general kernel's launch returned at once for them, fifty empty launches on the
        //  whole-genome job's phase 2)
        const bool walked = own == SW_GENERIC || own == SW_GENERIC64 || (!x.split && !(job->chunked && (x.lean || x.small || x.smallx || x.leanx)));
        k.general = walked ? own : SW_NONE;
        k.phase1 = k.lean ? (k.tri ? SW_LEAN_TRI : SW_LEAN) : k.leanx == 2u ? (k.widef ? SW_LEANX_TRIW : SW_LEANX_TRI) : k.leanx ? leanx_kernel
                 : k.small ? SW_SMALL16 : k.smallx ? SW_SMALL16X : k.tri ? SW_TRI1 : own;
        if (fused) k.phase2 = k.leanx2 ? SW_LEANX2 : k.tri == 2u ? SW_LEAN2 : k.small == 2u ? SW_SMALL16 : k.smallx == 2u ? SW_SMALL16X : own;
        else k.phase2 = k.lean ? SW_LEAN : k.leanx ? leanx_kernel : k.small ? SW_SMALL16 : k.smallx ? SW_SMALL16X : own;
        k.post = fused ? POST_NONE : job->persist ? POST_LOOP : POST_CHUNKS;
        // (k_bins_thin: what bins_thin() in pg_kernels.hip says — at most 64 partial entries per column, fused job)
        const BinsKernel own_bins = k.leanx2 ? BN_Q : (k.tri == 2u || k.cls4) ? BN_LEAN2 : (k.T <= 64u && x.HP <= 32u && fused) ? BN_THIN : BN_FULL;
        if (x.split) { k.bins = BN_S; k.bins_wide = (x.split == 2u && x.wide_bytes) ? BN_WIDE_S : BN_NONE; }
        else if (k.smallx == 2u) { k.bins = BN_X; k.bins_one = own_bins; k.bins_wide = x.wide_bytes ? BN_WIDE : BN_NONE; }
        else { k.bins = own_bins; k.bins_wide = (k.widef && x.n_wide_cand) ? BN_WIDE : BN_NONE; }

        job->hp_mask |= kSweep[k.phase1].bits | kSweep[k.phase2].bits | kSweep[k.general].bits;
        job->bins_which |= kBins[k.bins].bit | kBins[k.bins_one].bit | kBins[k.bins_wide].bit;
        if (a.params.run_phasing) job->vit_bits |= x.HP == 16 ? 1u : (x.HP == 32 ? 2u : 4u);
    }
    // the preparation beside phase 1 (pg_job::prep_beside): phase 1 in pieces, k_prep_bi the only emission kernel of the job — every
    // chain with variants all-biallelic without lists, none split —, and a piece left behind the E prepared ahead
    job->prep_beside = false; job->prep_early = 0; job->prep_W = 0; job->prep_parts_ready = false;
    if (job->n_pieces > 1u && !kc.prepahead) {
        bool only_bi = true;
        for (size_t c = 0; c < kernels.size(); ++c) if (job->index[a.specs[c].index].V && kernels[c].prep != PREP_BI) only_bi = false;
        uint32_t E = PG_PREP_EARLY_PIECES_DEFAULT;
        if (const char* e = getenv("PG_PREP_EARLY_PIECES")) { const long v = strtol(e, nullptr, 0); if (v >= 1 && v <= 0xFFFF) E = (uint32_t)v; }
        if (only_bi && job->n_pieces >= E + 1u) {
            job->prep_beside = true;
            job->prep_early = E;
            job->prep_W = pg_prep_band(job->n_pieces, E, job->piece_chunks * job->chunk_cols);
        }
    }
    return kernels;
}

std::string sweep_name(SweepKernel k, int phase) {
    const SweepRow& n = kSweep[k];
    return n.phased ? std::string(n.name) + "<" + std::to_string(phase) + ">" : std::string(n.name);
}

// the plan as text (pg_job_plan): one line per group of chains with the same kernels
std::string plan_text(const pg_job* job, const BuildArgs& a, const std::vector<ChainKernels>& kernels) {
    struct Group { std::string text; uint32_t count = 0; };
    std::vector<Group> groups;
    for (size_t c = 0; c < kernels.size(); ++c) {
        const IndexHost& x = job->index[a.specs[c].index];
        const ChainKernels& k = kernels[c];
        if (x.V == 0) continue;
        // (PG_KERNELS=generic: the text has always named the generic kernel for chains below 64 paths too, which it does not
        //  take — they run on k_sweep<HP>, as their launch bit says.  Kept: this text is what callers compare.)
        auto name = [&](SweepKernel s, int phase) { return sweep_name(a.kc.generic && s >= SW_HP16 && s <= SW_HP128 ? SW_GENERIC : s, phase); };
        std::string p2, bins;
        if (k.post == POST_LOOP) { p2 = name(k.phase2, 4) + " (one launch, all chunks) + k_post_loop"; bins = "(k_post_loop)"; }
        else if (k.post == POST_CHUNKS) { p2 = name(k.phase2, 3) + (k.sparse2 ? " chunks (sparse: every 64th column stored) + k_refill_lean (both halves) + " : k.sparse ? " chunks + k_refill_lean + " : " chunks + ") + "k_post"; bins = "(k_post)"; }
        else {
            p2 = name(k.phase2, 2);
            if (k.tri && k.phase2 == k.general) p2 += " (triangle ring)";
            if (k.widef) p2 += " (wide columns to their aux slots)";
            bins = kBins[k.bins].name;
            if (k.bins_wide) bins += std::string(" + ") + kBins[k.bins_wide].name;
        }
        char head[160];
        snprintf(head, sizeof(head), "%u path(s) (padded %u), %s%s%s columns: ", x.H, x.HP, x.pair_n > 2 ? "multiallelic" : "biallelic", x.wide_bytes ? " + wide" : "",
                 k.tri ? ", triangle" : "");
        const std::string text = std::string(head) + "prep = " + kPrepName[k.prep] + "; phase 1 = " + name(k.phase1, 1) + (k.sparse ? (k.sparse2 && job->n_pieces > 1u ? " (sparse: every 64th column stored, in " + std::to_string(job->n_pieces) + " pieces with k_refill_lean beside them)" : std::string(" (sparse: every 64th column stored)")) : std::string()) + "; phase 2 = " + p2 + "; bins = " + bins;
        bool found = false;
        for (auto& g : groups) if (g.text == text) { g.count += 1; found = true; break; }
        if (!found) groups.push_back({text, 1});
    }
    std::string out = std::string(job->chunked ? "chunked" : "fused") + " job, " + std::to_string(kernels.size()) + " chain(s)" + (a.params.run_phasing ? ", run_phasing (k_viterbi)" : "") +
                      (job->max_v == 0 || !a.params.run_genotyping ? std::string()
                       : job->prep_beside ? ", prep in parts: the ends of the chains ahead of the sweeps, their middle beside the first " + std::to_string(job->prep_early) + " of " +
                                            std::to_string(job->n_pieces) + " pieces (k_prep_bi_part, k_records_part; on the job's own stream)"
                                          : std::string(", prep ahead of the sweeps")) + "\n";   // (no word of a phase here: callers pick a chain group's line by those)
    for (const auto& g : groups) out += "  " + std::to_string(g.count) + " x " + g.text + "\n";
    return out;
}

// ---- the arena ------------------------------------------------------------------------------
// offsets of what the job as a whole and every chain own; those of an index contig's arrays are IndexHost's (o_*), a chain's
// sample arrays ChainHost's
struct ChainOffsets { size_t sync, wcols, wlist, aux, frec, scratch, wide, vpair, xbuf, prof, fback, fscale, bscale, bsum, vrec, colrec, fwd, part, cprec,
                      vtq, vback, vbest, hap1, hap2, ckpt; };
struct ArenaLayout {
    size_t o_contigs, o_reps, o_contigs_g, o_reps_g, o_small, o_dump, o_handshake, o_err, o_lik, o_likexp, o_ncols, o_ixerr;
    size_t zero_lo, zero_hi, ix_lo, ix_hi, vrec_lo, vrec_hi, srec_lo, srec_hi;   // the runs that are zeroed as one
    size_t bytes;
    std::vector<ChainOffsets> chain;
};

// Only arithmetic: where everything lies.  The ORDER of the take() calls is the layout — alignment and the zeroed runs hang on it.
ArenaLayout layout_arena(pg_job* job, const BuildArgs& a, const std::vector<ChainKernels>& kernels) {
    const uint32_t n_chains = (uint32_t)a.specs.size(), n_index = a.n_index;
    const bool vit = a.params.run_phasing != 0;
    const bool geno = a.params.run_genotyping != 0;  // (a phasing-only job has no sweep: no columns, no partials)
    ArenaLayout L;
    L.chain.resize(n_chains);
    size_t off = 0;
    auto take = [&](size_t bytes, size_t al = 256) { off = align_up(off, al); size_t o = off; off += (bytes ? bytes : 8); return o; };
    L.o_contigs = take(sizeof(DevContig) * n_chains);
    L.o_reps = take(sizeof(DevContig) * n_index);
    L.o_contigs_g = take(sizeof(DevContig) * n_chains); L.o_reps_g = take(sizeof(DevContig) * n_index);   // (the pipelined first run: group order)
    L.o_small = take(sizeof(uint32_t) * n_chains);   // chain ids of the H = 16 chains (k_sweep_small16)
    L.o_dump = take(64 * 8 * 16 + 8 * 16 * 16 * 16);  // scrap column for the stores of its rows that are done
    L.o_handshake = take(64);   // k_stream_handshake's words
    // zeroed-every-run block: n_cols, err, per chain kept / fallback flags / profile counters / allele_present,
    // then the packed lik and lik_exp regions (chain after chain, no gaps: one range each for a gather)
    L.zero_lo = align_up(off);
    L.o_err = take(sizeof(uint32_t) * n_chains);
    uint64_t lik_total = 0;
    for (uint32_t c = 0; c < n_chains; ++c) {
        ChainHost& ch = job->chains[c];
        const IndexHost& x = job->index[ch.index];
        ChainOffsets& p = L.chain[c];
        p.fback = take(x.V);
        p.prof = take(64 * sizeof(unsigned long long));
        p.wcols = take(4);   // (the count of the chain's wide-column list: zeroed with the rest of this block; the list itself below)
        p.sync = take(job->chunked ? PG_SYNC_WORDS * sizeof(uint32_t) : 0);   // (chunk hand-over words of the persistent phase 2)
        p.vbest = take(vit ? 4 : 0);
        p.hap1 = take(vit ? (size_t)x.V * 2 : 0);
        p.hap2 = take(vit ? (size_t)x.V * 2 : 0);
        ch.lik_first = lik_total;
        lik_total += x.n_lik;
    }
    job->n_lik_total = lik_total;
    L.o_lik = take(lik_total * sizeof(double));
    L.o_likexp = take(lik_total * sizeof(int32_t));
    L.zero_hi = off;
    job->o_tab_m = take(job->tab_m.size() * sizeof(double));
    job->o_tab_e = take(job->tab_e.size() * sizeof(int32_t));
    job->o_tab_p = take(job->tab_p.size());
    // what the index alone decides, formed by the index-level kernels whenever an index is uploaded (pg_split.h): one run of the
    // arena, zeroed before every such pass — column flags, present alleles, the column list and its inverse for every index
    // contig; for split contigs the per-column records and the list of wide columns
    L.ix_lo = align_up(off);
    L.o_ncols = take(sizeof(uint32_t) * n_index);
    L.o_ixerr = take(sizeof(uint32_t) * n_index);
    for (IndexHost& x : job->index) {
        x.o_kept = take(x.V); x.o_apres = take(x.sumA);
        x.o_colv = take((size_t)x.V * 4); x.o_colof = take((size_t)x.V * 4);
        x.o_ixpd = take(x.split ? (size_t)x.V * PG_IXPD_BYTES : 0);
        x.o_ixrec = take(x.split ? (size_t)x.V * PG_IXREC_BYTES : 0);
        x.o_ixbin = take(x.split ? (size_t)x.V * PG_IXBIN_BYTES : 0);
        x.o_ixwl = take(x.split == 2u && x.wide_bytes ? (size_t)x.n_wide_cand * 4 : 0);
        x.o_ixnw = take(4);
    }
    L.ix_hi = off > L.ix_lo ? off : L.ix_lo;
    for (IndexHost& x : job->index) {
        x.o_pos = take((size_t)x.V * 8);
        x.o_koff = take(((size_t)x.V + 1) * 4);
        x.o_aoff = take(((size_t)x.V + 1) * 4); x.o_aid = take((size_t)x.sumA * 2);
        x.o_aflag = take(x.sumA); x.o_akoff = take((size_t)x.sumA * 2); x.o_akmask = take((size_t)x.sumA * 4);
        x.o_pa = take((size_t)x.V * x.H * 2);
        x.o_goff = take(((size_t)x.V + 1) * 8);
        x.o_widx = take(x.wide_bytes ? (size_t)x.V * 4 : 0);
        x.o_auxidx = take(x.aux_bytes ? (size_t)x.V * 4 : 0);
        x.o_list_m4 = take(x.list_m4.size() * 4);
        x.o_list_w = take(x.list_w.size() * 4);
        x.o_list_b = take(x.list_b.size() * 4);
        x.o_list_big = take(x.list_big.size() * 4);
    }
    job->sample_lo = align_up(off);   // the per-sample arrays of all chains, one contiguous run (pg_job::sample_lo)
    for (ChainHost& ch : job->chains) {
        const IndexHost& x = job->index[ch.index];
        ch.o_cov = take((size_t)x.V * 2); ch.o_kcnt = take((size_t)x.sumK * 2);
    }
    job->sample_bytes = align_up(off) - job->sample_lo;
    // The variant records of all chains in ONE run of the arena, zeroed once when the job is built: k_prep_bi writes only the
    // pieces of a biallelic object's record that are not zero by construction (header, row bits, four table entries, the path
    // alleles: 96 of 384 bytes at 16 paths — it is a kernel that waits for its memory 70 % of the time); what it leaves out — the
    // rest of the 6 x 6 table, the padding — has to BE zero for every reader of the full record.
    L.vrec_lo = align_up(off);
    for (uint32_t c = 0; c < n_chains; ++c) { const IndexHost& x = job->index[job->chains[c].index]; L.chain[c].vrec = take(x.split ? 0 : (size_t)x.V * x.RB); }
    L.vrec_hi = off;
    // ... and the sample records of the split chains in another: zeroed with every index pass (k_prep_s_bi stores only the pieces
    // of a biallelic column's 128-byte record that are not zero by construction; which columns those are hangs on the index alone)
    L.srec_lo = align_up(off);
    for (uint32_t c = 0; c < n_chains; ++c) {
        const IndexHost& x = job->index[job->chains[c].index];
        if (x.split) L.chain[c].frec = take((size_t)x.V * (x.split == 1u ? PG_SREC1_BYTES : PG_SREC2_BYTES));
    }
    L.srec_hi = off > L.srec_lo ? off : L.srec_lo;   // (no split chain: an empty run)
    for (uint32_t c = 0; c < n_chains; ++c) {
        const IndexHost& x = job->index[job->chains[c].index];
        const ChainKernels& k = kernels[c];
        ChainOffsets& p = L.chain[c];
        p.colrec = take(x.split ? 0 : (size_t)x.V * x.RB);
        p.cprec = take(x.split ? (size_t)x.V * PG_CPREC_BYTES : 0);
        p.fwd = take(geno ? (size_t)x.V * (k.tri ? 2304u : (size_t)x.HP * x.HP) * sizeof(double) : 0);   // (triangle chains: 2304 doubles per column)
        // fused mode: posterior partials; chunked mode: the chunk scratch instead (k_post writes lik directly)
        // (x chains of fused jobs: four class sums per column — plus the per-thread partials of ONE column, should the chain
        //  be left with a single column and run its phase 2 on the general kernel)
        const bool x2 = k.smallx == 2u;
        p.part = take(job->chunked || !geno ? 0 : (x2 ? (size_t)x.V * 32u + (size_t)x.part_slots * part_entries(x) * sizeof(double)
                                                      : (size_t)x.V * x.part_slots * part_entries(x) * sizeof(double)));
        p.aux = take((x2 || x.widef) && geno ? x.aux_bytes : 0);
        p.wlist = take((x2 || x.widef) && geno && x.wide_bytes && !x.split ? (size_t)x.n_wide_cand * 4 : 0);
        // Viterbi: transition probabilities and one 2-byte backpointer per state and column
        p.vtq = take(vit ? (size_t)x.V * 8 * sizeof(double) : 0);
        p.vback = take(vit ? (size_t)x.V * x.H * x.HP * sizeof(uint16_t) : 0);
        p.scratch = take(job->chunked ? (size_t)2 * PG_SCRATCH_BUFS * job->chunk_cols * x.HP * x.HP * sizeof(double) : 0);
        // (sparse phase 2: every checkpoint of the chain's phase 2, never reused within a run)
        p.ckpt = take(k.sparse2 ? (size_t)2 * pg_sparse2_slots(x.V) * x.HP * x.HP * sizeof(double) : 0);
        p.wide = take(x.wide_bytes);
        p.vpair = take(x.split ? 0 : (size_t)x.V * pg_pair_bytes(x.pair_n));
        p.xbuf = take((x.HP >= 256 || (a.kc.generic && x.HP >= 64)) ? (size_t)2 * x.HP * x.HP * sizeof(double) : 0);
        if (!x.split) p.frec = take((x.lean || x.small) ? (size_t)x.V * 64 : (x.smallx ? (size_t)x.V * 192 : 0));
        p.fscale = take((size_t)x.V * sizeof(double));
        p.bscale = take((size_t)x.V * sizeof(double));
        p.bsum = take((size_t)x.V * sizeof(double));
    }
    L.bytes = align_up(off);
    return L;
}

// The arena: from the process pool (one-shot jobs), else hipMalloc — once more after the pool has been emptied.
hipError_t allocate_arena(pg_job* job, size_t bytes) {
    const double t0 = now_s();
    job->arena_bytes = bytes;
    if (job->cache_arena) g_pool.take(job->device, job->arena_bytes, &job->arena, &job->arena_bytes);
    hipError_t he = hipSuccess;
    if (!job->arena) {
        he = hipMalloc((void**)&job->arena, job->arena_bytes);
        if (he != hipSuccess) {
            (void)hipGetLastError();
            pg_hmm_release_cache();  // cached arenas may be what stands in the way
            hipSetDevice(job->device);
            he = hipMalloc((void**)&job->arena, job->arena_bytes);
        }
        if (he != hipSuccess) { job->arena = nullptr; (void)hipGetLastError(); }
    }
    job->host_s[0] = now_s() - t0;
    return he;
}

// the job's streams and events; the second stream and the chunk events for chunked jobs only
int create_device_objects(pg_job* job, char* err, size_t errlen) {
    hipError_t he;
    if ((he = hipStreamCreate(&job->stream)) != hipSuccess) return hip_fail(err, errlen, "hipStreamCreate", he);
    for (auto& e : job->ev)
        if ((he = hipEventCreate(&e)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
    for (auto& e : job->ev_vit)
        if ((he = hipEventCreate(&e)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
    for (auto& e : job->ev_ix)
        if ((he = hipEventCreate(&e)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
    job->events = true;
    if (!job->chunked) return PG_OK;
    if ((he = hipStreamCreateWithFlags(&job->stream2, hipStreamNonBlocking)) != hipSuccess) return hip_fail(err, errlen, "hipStreamCreate", he);
    for (int q = 0; q < (int)PG_SCRATCH_BUFS; ++q) {
        if ((he = hipEventCreateWithFlags(&job->ev_sweep[q], hipEventDisableTiming)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
        if ((he = hipEventCreateWithFlags(&job->ev_post[q], hipEventDisableTiming)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
    }
    job->events2 = true;
    if (job->sparse2) {
        job->ev_chunk.reserve(job->n_chunks);
        for (uint32_t q = 0; q < job->n_chunks; ++q) {
            hipEvent_t e;
            if ((he = hipEventCreateWithFlags(&e, hipEventDisableTiming)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
            job->ev_chunk.push_back(e);
        }
        if (job->n_pieces > 1u) for (uint32_t g = 0; g < job->n_pieces; ++g) {
            hipEvent_t e;
            if ((he = hipEventCreateWithFlags(&e, hipEventDisableTiming)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
            job->ev_piece.push_back(e);
        }
        if (job->prep_beside && (he = hipEventCreateWithFlags(&job->ev_prep2, hipEventDisableTiming)) != hipSuccess) return hip_fail(err, errlen, "hipEventCreate", he);
    }
    return PG_OK;
}

// the job's pointers into its arena
void bind_arena(pg_job* job, const ArenaLayout& L) {
    unsigned char* A = job->arena;
    job->d_contigs = (DevContig*)(A + L.o_contigs);
    job->d_reps = (DevContig*)(A + L.o_reps);
    job->d_contigs_g = (DevContig*)(A + L.o_contigs_g); job->d_reps_g = (DevContig*)(A + L.o_reps_g);
    job->d_small = (uint32_t*)(A + L.o_small);
    job->d_dump = (double*)(A + L.o_dump);
    job->d_handshake = (uint32_t*)(A + L.o_handshake);
    job->d_ixerr = (uint32_t*)(A + L.o_ixerr);
    job->ix_base = A + L.ix_lo; job->ix_bytes = L.ix_hi - L.ix_lo;
    job->srec_base = A + L.srec_lo; job->srec_bytes = L.srec_hi - L.srec_lo;
    job->d_ncols = (uint32_t*)(A + L.o_ncols);
    job->d_err = (uint32_t*)(A + L.o_err);
    job->d_lik = (double*)(A + L.o_lik);
    job->d_likexp = (int32_t*)(A + L.o_likexp);
    job->zero_base = A + L.zero_lo;
    job->zero_bytes = L.zero_hi - L.zero_lo;
    job->tab.mant = (const double*)(A + job->o_tab_m);
    job->tab.expo = (const int32_t*)(A + job->o_tab_e);
    job->tab.packed = A + job->o_tab_p;
    job->cur_samples = A + job->sample_lo;
}

// One DevContig per chain from the offsets and the chain's kernels, and the grid extents of the kernels that walk lists.
std::vector<DevContig> fill_descriptors(pg_job* job, const BuildArgs& a, const std::vector<ChainKernels>& kernels, const ArenaLayout& L) {
    unsigned char* A = job->arena;
    const pg_hmm_params& params = a.params;
    std::vector<DevContig> hd(job->chains.size());
    const long double dist_scale = 0.000004L * ((long double)params.recombrate) * params.effective_N;
    for (size_t c = 0; c < hd.size(); ++c) {
        ChainHost& ch = job->chains[c];
        const IndexHost& x = job->index[ch.index];
        const ChainOffsets& p = L.chain[c];
        const ChainKernels& k = kernels[c];
        DevContig& d = hd[c];
        memset(&d, 0, sizeof(d));
        d.V = x.V; d.H = x.H; d.HP = x.HP; d.RB = x.RB; d.T = k.T; d.part_slots = x.part_slots; d.pair_n = x.pair_n;
        d.dist_scale = (double)dist_scale; d.uniform = params.uniform ? 1 : 0;
        d.debug = 8u;   // (bit 3: the in-kernel cycle counters of -DPG_CHAIN_PROF builds; the product build has none)
        d.pos = (const uint64_t*)(A + x.o_pos); d.cov = (const uint16_t*)(A + ch.o_cov);
        d.kmer_off = (const uint32_t*)(A + x.o_koff); d.kmer_count = (const uint16_t*)(A + ch.o_kcnt);
        d.allele_off = (const uint32_t*)(A + x.o_aoff); d.allele_id = (const uint16_t*)(A + x.o_aid);
        d.allele_flags = (const uint8_t*)(A + x.o_aflag); d.allele_koff = (const uint16_t*)(A + x.o_akoff);
        d.allele_kmask = (const uint32_t*)(A + x.o_akmask); d.path_allele = (const uint16_t*)(A + x.o_pa);
        d.geno_off = (const uint64_t*)(A + x.o_goff);
        d.vrec = A + p.vrec; d.kept = A + x.o_kept; d.allele_present = A + x.o_apres;
        d.n_cols = job->d_ncols + ch.index; d.col_variant = (uint32_t*)(A + x.o_colv); d.colrec = A + p.colrec;
        d.col_of = (const uint32_t*)(A + x.o_colof); d.ix_err = job->d_ixerr + ch.index;
        d.ix_big = (const uint32_t*)(A + x.o_list_big); d.n_ix_big = (uint32_t)x.list_big.size();
        d.split = x.split;
        if (x.split) {
            d.ix_pd = A + x.o_ixpd; d.ix_rec = A + x.o_ixrec; d.ix_bin = A + x.o_ixbin; d.cprec = A + p.cprec;
        }
        d.fwd = (double*)(A + p.fwd); d.part = (double*)(A + p.part); d.fwd_fallback = A + p.fback; d.prof = (unsigned long long*)(A + p.prof);
        d.fscale = (double*)(A + p.fscale); d.bscale = (double*)(A + p.bscale); d.bsum = (double*)(A + p.bsum); d.err = job->d_err + c;
        d.lik = job->d_lik + ch.lik_first; d.lik_exp = job->d_likexp + ch.lik_first;
        d.scratch = (double*)(A + p.scratch); d.chunk_cols = job->chunk_cols; d.sync = (uint32_t*)(A + p.sync);
        d.wide = A + p.wide; d.wide_idx = x.wide_bytes ? (const uint32_t*)(A + x.o_widx) : nullptr;
        d.vpair = A + p.vpair; d.xbuf = (double*)(A + p.xbuf);
        d.frec = (double*)(A + p.frec);
        d.lean = k.lean; d.small = k.small; d.smallx = k.smallx; d.leanx = k.leanx; d.leanx2 = k.leanx2; d.cls4 = k.cls4; d.widef = k.widef; d.tri = k.tri; d.sparse = k.sparse;
        d.sparse2 = k.sparse2; d.ckpt = (double*)(A + p.ckpt); d.ckpt_slots = pg_sparse2_slots(x.V);
        d.col_stride = d.tri ? 2304u : x.HP * x.HP;
        d.aux = A + p.aux; d.aux_idx = ((d.smallx == 2u || x.widef) && x.aux_bytes) ? (const uint32_t*)(A + x.o_auxidx) : nullptr;
        if ((d.smallx == 2u || x.widef) && x.wide_bytes && x.n_wide_cand) {
            // (split chains: the wide columns hang on the index alone — one list per index contig, made by k_index_cols)
            if (x.split) { d.wcols = (uint32_t*)(A + x.o_ixwl); d.n_wcols = (uint32_t*)(A + x.o_ixnw); }
            else { d.wcols = (uint32_t*)(A + p.wlist); d.n_wcols = (uint32_t*)(A + p.wcols); }
            job->max_wide = std::max(job->max_wide, x.n_wide_cand);
        }
        d.live = (!job->chunked && x.HP == 32u && !a.kc.fullcols) ? std::min<uint32_t>(x.HP, (x.H + 3u) & ~3u) : x.HP;
        d.prep_fast = x.prep_fast;
        // who walks lists: the split path's emission kernels unless every object is k_prep_s_bi's, the others when only a part
        // of the objects is k_prep_bi's (a non-null list pointer = "walk the list", also when it is empty)
        if (k.prep == PREP_S_LISTS || k.prep == PREP_BI_LISTS) {
            d.prep_m4 = (const uint32_t*)(A + x.o_list_m4); d.n_prep_m4 = (uint32_t)x.list_m4.size();
            d.prep_w = (const uint32_t*)(A + x.o_list_w); d.n_prep_w = (uint32_t)x.list_w.size();
            d.prep_b = (const uint32_t*)(A + x.o_list_b); d.n_prep_b = (uint32_t)x.list_b.size();
        }
        if (x.split) {
            job->max_sb = std::max(job->max_sb, k.prep == PREP_S_BI ? x.V : d.n_prep_b);
            job->max_sm4 = std::max(job->max_sm4, d.n_prep_m4);
            job->max_sw = std::max(job->max_sw, d.n_prep_w);
        } else {
            job->any_legacy_prep = true;
            job->max_prep_m4 = std::max(job->max_prep_m4, d.n_prep_m4);
            job->max_prep_w = std::max(job->max_prep_w, k.prep == PREP_W ? x.V : d.n_prep_w);
        }
        if (params.run_phasing) {
            d.vit_tq = (double*)(A + p.vtq); d.vit_back = (uint16_t*)(A + p.vback); d.vit_best = (uint32_t*)(A + p.vbest);
            d.hap1 = (uint16_t*)(A + p.hap1); d.hap2 = (uint16_t*)(A + p.hap2);
        }
        ch.d = d;
    }
    return hd;
}

// What the kernels read of the job itself goes to the device: the variant records' zeroes, the chain-id lists of the
// four-half-chains-per-wave kernels, one descriptor per index contig, the chain descriptors.
int upload_descriptors(pg_job* job, const ArenaLayout& L, const std::vector<DevContig>& hd, char* err, size_t errlen) {
    hipError_t he;
    hipStream_t s = job->stream;
    const uint32_t n_chains = (uint32_t)hd.size(), n_index = (uint32_t)job->index.size();
    if ((he = hipMemsetAsync(job->arena + L.vrec_lo, 0, L.vrec_hi - L.vrec_lo, s)) != hipSuccess) return hip_fail(err, errlen, "hipMemset (variant records)", he);
    // chain ids: the all-biallelic chains first, then the x chains; each list in the order of the index contigs (stable), so that
    // the four rows of a wave are — in a cohort — samples of ONE contig: the same columns are multiallelic / wide in all four
    // (the wide branch of k_sweep_small16x is wave-uniform)
    std::vector<uint32_t> small_ids, x_ids;
    for (uint32_t c = 0; c < n_chains; ++c) {
        if (hd[c].small) { small_ids.push_back(c); if (hd[c].small == 2u) job->small_phase2 = true; }
        if (hd[c].smallx) { x_ids.push_back(c); if (hd[c].smallx == 2u) job->smallx_phase2 = true; }
    }
    auto by_index = [&](uint32_t p, uint32_t q) { return job->chains[p].index < job->chains[q].index; };
    std::stable_sort(small_ids.begin(), small_ids.end(), by_index);
    std::stable_sort(x_ids.begin(), x_ids.end(), by_index);
    job->n_small = (uint32_t)small_ids.size();
    job->n_smallx = (uint32_t)x_ids.size();
    job->d_smallx = job->d_small + job->n_small;
    small_ids.insert(small_ids.end(), x_ids.begin(), x_ids.end());
    if (!small_ids.empty() && ((he = hipMemcpyAsync(job->d_small, small_ids.data(), sizeof(uint32_t) * small_ids.size(), hipMemcpyHostToDevice, s)) != hipSuccess ||
                               (he = hipStreamSynchronize(s)) != hipSuccess))
        return hip_fail(err, errlen, "hipMemcpy small ids", he);
    // one descriptor per index contig for the index-level kernels (any chain over it: they touch index-level fields only)
    std::vector<DevContig> reps(n_index);
    for (auto& r : reps) memset(&r, 0, sizeof(r));
    std::vector<char> have(n_index, 0);
    for (uint32_t c = 0; c < n_chains; ++c) { const uint32_t i = job->chains[c].index; if (!have[i]) { have[i] = 1; reps[i] = hd[c]; } }
    if ((he = hipMemcpyAsync(job->d_reps, reps.data(), sizeof(DevContig) * n_index, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (he = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(err, errlen, "hipMemcpy index descriptors", he);
    if ((he = hipMemcpyAsync(job->d_contigs, hd.data(), sizeof(DevContig) * n_chains, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (he = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(err, errlen, "hipMemcpy contigs", he);
    job->h_contigs = hd;
    return PG_OK;
}

// The pipelined first run (pg_job::pipeline): a one-shot job — upload and run inside one call — of few chains (chunked: bound
// by its longest chain, not by throughput), every chain over an index contig of its own, on kernels that take a sub-range
// of the descriptor array (no chain-id lists, no split path), with enough bytes to upload that hiding them matters.
// Group A = the chains with at least 0.78 of the longest one's variants (they decide the wall time; the others, starting
// later by their upload — ~10 % of a run at 40 GB/s —, still end phase 1 first), unless that is most of the bytes anyway.
int plan_pipeline(pg_job* job, const BuildArgs& a, const std::vector<DevContig>& hd, char* err, size_t errlen) {
    const uint32_t n_chains = (uint32_t)hd.size();
    bool ok = job->chunked && !a.cohort && a.n_index == n_chains && n_chains >= 2 && !job->any_split &&
              a.params.run_genotyping && !a.params.run_phasing && getenv("PG_NO_PIPELINE") == nullptr;
    for (uint32_t c = 0; ok && c < n_chains; ++c) ok = job->chains[c].index == c && !job->index[c].small && !job->index[c].smallx;
    if (!ok) return PG_OK;
    uint64_t vmax = 0, wA = 0, wAll = 0;
    for (const IndexHost& x : job->index) vmax = std::max<uint64_t>(vmax, x.V);
    std::vector<uint32_t> ga, gb;
    for (uint32_t c = 0; c < n_chains; ++c) {
        const IndexHost& x = job->index[c];
        const uint64_t w = (uint64_t)x.V * x.H * 2u + (uint64_t)x.sumK * 2u + (uint64_t)x.V * 24u;
        wAll += w;
        if ((double)x.V >= 0.78 * (double)vmax) { ga.push_back(c); wA += w; } else gb.push_back(c);
    }
    uint64_t min_bytes = (uint64_t)128 << 20;   // (PG_PIPELINE_MIN_MB: tests put small jobs through the pipelined run)
    if (const char* e = getenv("PG_PIPELINE_MIN_MB")) min_bytes = (uint64_t)strtoul(e, nullptr, 0) << 20;
    if (gb.empty() || wAll < min_bytes || (double)wA > 0.6 * (double)wAll) return PG_OK;
    job->grp_order = ga;
    job->grp_order.insert(job->grp_order.end(), gb.begin(), gb.end());
    job->nA = (uint32_t)ga.size();
    std::vector<DevContig> g(n_chains);
    for (uint32_t k = 0; k < n_chains; ++k) g[k] = hd[job->grp_order[k]];
    // (chain c over index c: the chain's descriptor serves as its index contig's)
    hipError_t he;
    if ((he = hipMemcpyAsync(job->d_contigs_g, g.data(), sizeof(DevContig) * n_chains, hipMemcpyHostToDevice, job->stream)) != hipSuccess ||
        (he = hipMemcpyAsync(job->d_reps_g, g.data(), sizeof(DevContig) * n_chains, hipMemcpyHostToDevice, job->stream)) != hipSuccess ||
        (he = hipStreamSynchronize(job->stream)) != hipSuccess)
        return hip_fail(err, errlen, "hipMemcpy group descriptors", he);
    if (hipEventCreateWithFlags(&job->ev_late[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&job->ev_late[1], hipEventDisableTiming) == hipSuccess) {
        job->ev_late_made = true;
        job->pipeline_capable = true;
        job->pipeline = a.cache_arena;   // (a resident job's first upload returns to a caller who may free the arrays: pg_job_upload_run asks for it)
    }
    return PG_OK;
}

int job_build(int device, uint32_t n_index, const pg_contig_batch* batches, const std::vector<ChainSpec>& specs,
              uint32_t n_samples, bool cohort, const pg_table* table, const pg_hmm_params* params, bool cache_arena,
              pg_job** out, char* err, size_t errlen) {
    *out = nullptr;
#ifdef PG_HOST_TIMING   // (measurement builds: where the host time of a job's construction goes)
    double tb_last = now_s();
    auto lap = [&](const char* what) { const double t = now_s(); fprintf(stderr, "[job_build] %-28s %8.3f ms\n", what, (t - tb_last) * 1e3); tb_last = t; };
#else
    auto lap = [](const char*) {};
#endif
    int rc = check_inputs(n_index, batches, specs, table, params, cohort, err, errlen);
    if (rc == PG_OK) rc = select_device(device, err, errlen);
    if (rc != PG_OK) return rc;
    lap("checks");
    const BuildArgs a{n_index, batches, specs, *params, kernel_choice(), cohort, cache_arena};
    if (!a.kc.unknown.empty()) { set_err(err, errlen, "PG_KERNELS: unknown token '%s'", a.kc.unknown.c_str()); return PG_ERR_INVALID; }
    JobOwner owner{new pg_job()};
    pg_job* job = owner.job;
    job->device = device;
    job->params = *params;
    job->cache_arena = cache_arena;
    job->cohort = cohort;
    job->n_samples = n_samples;
    job->n_contigs = n_index;
    job->chains.resize(specs.size());
    for (size_t c = 0; c < specs.size(); ++c) job->chains[c].index = specs[c].index;
    table_snapshot(const_cast<pg_table*>(table), job->tab_m, job->tab_e, job->tab_p, &job->tab);
    lap("table");
    if ((rc = classify_index(job, a, err, errlen)) != PG_OK) return rc;
    lap("index classification");
    // A chunked job's scratch (PG_SCRATCH_BUFS buffers of chunk_cols columns per half-chain: up to choose_job_mode's 39 GB budget) is a choice, not a need:
    // before giving up, plan again with half the chunk columns, down to 64 (the fixed budget could fail a job that
    // fitted with smaller chunks — on a smaller device, or next to other resident jobs)
    std::vector<ChainKernels> kernels;
    ArenaLayout L;
    hipError_t he = hipSuccess;
    for (size_t chunk_cap = 0;; chunk_cap = job->chunk_cols / 2u) {
        choose_job_mode(job, a, chunk_cap);
        kernels = choose_chain_kernels(job, a);
        L = layout_arena(job, a, kernels);
        he = allocate_arena(job, L.bytes);
        if (he == hipSuccess || !job->chunked || job->chunk_cols <= 64u) break;
    }
    if (he != hipSuccess) { set_err(err, errlen, "hipMalloc(%zu bytes) failed: %s", L.bytes, hipGetErrorString(he)); return PG_ERR_NOMEM; }
    lap("mode, kernels, arena");
    if ((rc = create_device_objects(job, err, errlen)) != PG_OK) return rc;
    lap("streams, events");
    bind_arena(job, L);
    const std::vector<DevContig> hd = fill_descriptors(job, a, kernels, L);
    job->plan_text = plan_text(job, a, kernels);
    if ((rc = upload_descriptors(job, L, hd, err, errlen)) != PG_OK) return rc;
    lap("descriptors");
    if ((rc = plan_pipeline(job, a, hd, err, errlen)) != PG_OK) return rc;
    if ((rc = upload_inputs(job, batches, specs, true, err, errlen)) != PG_OK) return rc;
    lap("upload of the inputs");
    *out = owner.release();
    return PG_OK;
}

// The chains of a cohort, sample-major: chain s * n_contigs + c reads sample s's arrays of contig c.
int cohort_chain_specs(uint32_t n_samples, uint32_t n_contigs, const pg_sample_counts* samples, std::vector<ChainSpec>& specs,
                       char* err, size_t errlen) {
    specs.resize((size_t)n_samples * n_contigs);
    for (uint32_t s = 0; s < n_samples; ++s) {
        if (!samples[s].kmer_count || !samples[s].coverage) { set_err(err, errlen, "sample %u has null arrays", s); return PG_ERR_INVALID; }
        for (uint32_t c = 0; c < n_contigs; ++c)
            specs[(size_t)s * n_contigs + c] = {c, samples[s].kmer_count[c], samples[s].coverage[c]};
    }
    return PG_OK;
}

// No chain of a resident job that has variants may come with null arrays: the first such chain is refused by its number.
int check_chain_arrays(const pg_job* job, const std::vector<ChainSpec>& specs, char* err, size_t errlen) {
    for (size_t c = 0; c < specs.size(); ++c) {
        const IndexHost& x = job->index[job->chains[c].index];
        if (x.V > 0 && (!specs[c].coverage || (x.sumK > 0 && !specs[c].kmer_count))) {
            set_err(err, errlen, "chain %zu has null kmer_count / coverage arrays", c);
            return PG_ERR_INVALID;
        }
    }
    return PG_OK;
}

}  // namespace

extern "C" int pg_job_new(int device, uint32_t n_contigs, const pg_contig_batch* batches, const pg_table* table,
                          const pg_hmm_params* params, pg_job** out, char* err, size_t errlen) {
    if (!out) { set_err(err, errlen, "null argument"); return PG_ERR_INVALID; }
    *out = nullptr;
    if (!batches || n_contigs == 0) { set_err(err, errlen, "null argument"); return PG_ERR_INVALID; }
    std::vector<ChainSpec> specs(n_contigs);
    for (uint32_t i = 0; i < n_contigs; ++i) specs[i] = {i, batches[i].kmer_count, batches[i].coverage};
    return job_build(device, n_contigs, batches, specs, 1, false, table, params, false, out, err, errlen);
}

extern "C" pg_job* pg_job_create(int device, uint32_t n_contigs, const pg_contig_batch* batches,
                                 const pg_table* table, const pg_hmm_params* params, char* err, size_t errlen) {
    pg_job* job = nullptr;
    pg_job_new(device, n_contigs, batches, table, params, &job, err, errlen);
    return job;
}

extern "C" int pg_cohort_new(int device, uint32_t n_contigs, const pg_contig_batch* index, uint32_t n_samples,
                             const pg_sample_counts* samples, const pg_table* table, const pg_hmm_params* params,
                             pg_job** out, char* err, size_t errlen) {
    if (!out) { set_err(err, errlen, "null argument"); return PG_ERR_INVALID; }
    *out = nullptr;
    if (!index || !samples || n_contigs == 0 || n_samples == 0) { set_err(err, errlen, "null argument"); return PG_ERR_INVALID; }
    std::vector<ChainSpec> specs;
    const int rc = cohort_chain_specs(n_samples, n_contigs, samples, specs, err, errlen);
    if (rc != PG_OK) return rc;
    return job_build(device, n_contigs, index, specs, n_samples, true, table, params, false, out, err, errlen);
}

extern "C" int pg_job_upload_run(pg_job* job, const pg_contig_batch* batches, const pg_sample_counts* samples, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    // upload + run inside ONE call: the host arrays stay valid throughout, so the upload of the shorter chains may hide behind
    // the long chains' phase 1 (pg_job::pipeline) where the job is capable of it; otherwise exactly pg_job_upload, pg_job_run
    job->pipeline = job->pipeline_capable && batches != nullptr && getenv("PG_NO_PIPELINE") == nullptr;
    int rc = pg_job_upload(job, batches, samples, err, errlen);
    job->pipeline = false;
    if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, errlen);
    return rc;
}

extern "C" int pg_job_upload(pg_job* job, const pg_contig_batch* batches, const pg_sample_counts* samples, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (job->upload_pending) { set_err(err, errlen, "an asynchronous upload is in flight: call pg_job_upload_end first"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    const uint32_t n = (uint32_t)job->chains.size();
    std::vector<ChainSpec> specs(n);
    if (batches)  // the layout must be the one the arena, the genotype / wide offsets and the kernel choice were planned for:
        for (uint32_t i = 0; i < job->n_contigs; ++i) {  // per-variant K and A, not just their totals
            const IndexHost& x = job->index[i];
            const int rc = check_batch(&batches[i], !job->cohort, err, errlen);
            if (rc != PG_OK) return rc;
            if (batches[i].n_variants != x.V || batches[i].n_paths != x.H ||
                (x.V && (memcmp(batches[i].kmer_off, x.koff.data(), ((size_t)x.V + 1) * 4) != 0 ||
                         memcmp(batches[i].allele_off, x.aoff.data(), ((size_t)x.V + 1) * 4) != 0))) {
                set_err(err, errlen, "contig %u: shape (variants, paths, k-mers or alleles per variant) differs from the resident job", i);
                return PG_ERR_INVALID;
            }
        }
    if (job->cohort) {
        if (!samples) { set_err(err, errlen, "cohort job: samples must be given"); return PG_ERR_INVALID; }
        const int rc = cohort_chain_specs(job->n_samples, job->n_contigs, samples, specs, err, errlen);
        if (rc != PG_OK) return rc;
    } else {
        if (!batches) { set_err(err, errlen, "batches must be given"); return PG_ERR_INVALID; }
        for (uint32_t i = 0; i < n; ++i) specs[i] = {i, batches[i].kmer_count, batches[i].coverage};
    }
    const int rc = check_chain_arrays(job, specs, err, errlen);
    if (rc != PG_OK) return rc;
    return upload_inputs(job, batches, specs, batches != nullptr, err, errlen);
}

// The next batch of samples of a cohort job, uploaded WHILE the current one is being genotyped: a worker thread packs
// the counts into the pinned staging buffer and copies them into the job's second set of per-sample arrays on a copy
// stream of its own; pg_job_upload_end waits for it and makes that set the one pg_job_run reads.  The caller's arrays
// must stay valid (and unchanged) until pg_job_upload_end returns.
extern "C" int pg_job_upload_begin(pg_job* job, const pg_sample_counts* samples, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (job->upload_pending) { set_err(err, errlen, "an upload is already in flight: call pg_job_upload_end first"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    if (!job->cohort) { set_err(err, errlen, "not a cohort job"); return PG_ERR_INVALID; }
    if (!samples) { set_err(err, errlen, "cohort job: samples must be given"); return PG_ERR_INVALID; }
    auto specs = std::make_shared<std::vector<ChainSpec>>();
    int rc = cohort_chain_specs(job->n_samples, job->n_contigs, samples, *specs, err, errlen);
    if (rc == PG_OK) rc = check_chain_arrays(job, *specs, err, errlen);
    if (rc != PG_OK) return rc;
    const size_t n = job->chains.size();
    if (!job->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&job->copy_stream, hipStreamNonBlocking));
    if (!job->alt_samples) {   // the second set + descriptors that point into it
        hipError_t he = hipMalloc((void**)&job->alt_samples, job->sample_bytes ? job->sample_bytes : 8);
        if (he != hipSuccess) {   // cached arenas of finished one-shot calls may be what stands in the way (as in job_build)
            (void)hipGetLastError();
            job->alt_samples = nullptr;
            pg_hmm_release_cache();
            hipSetDevice(job->device);
            he = hipMalloc((void**)&job->alt_samples, job->sample_bytes ? job->sample_bytes : 8);
        }
        if (he == hipSuccess) he = hipMalloc((void**)&job->d_contigs_owned, sizeof(DevContig) * n);
        job->d_contigs_alt = job->d_contigs_owned;
        if (he != hipSuccess) {
            if (job->alt_samples) { hipFree(job->alt_samples); job->alt_samples = nullptr; }
            job->d_contigs_alt = job->d_contigs_owned = nullptr;
            set_err(err, errlen, "hipMalloc (second sample set, %zu bytes) failed: %s", job->sample_bytes, hipGetErrorString(he));
            return PG_ERR_NOMEM;
        }
    }
    unsigned char* other = job->cur_samples == job->alt_samples ? job->arena + job->sample_lo : job->alt_samples;
    DevContig* d_other = job->d_contigs_alt;   // (the spare descriptor array: pg_job_upload_end swaps the two)
    job->next_coverage.assign(n, {});
    job->upload_pending = true;
    job->upload_rc = PG_OK;
    job->upload_err.clear();
    if (job->uploader.joinable()) job->uploader.join();
    job->uploader = std::thread([job, specs, other, d_other, n]() {
        char e[256] = {0};
        uint64_t bytes = 0;
        int r = hipSetDevice(job->device) == hipSuccess ? PG_OK : PG_ERR_DEVICE;
        if (r == PG_OK) r = sample_upload(job, *specs, other, job->copy_stream, &job->next_coverage, &bytes, e, sizeof(e));
        if (r == PG_OK) {   // the descriptors of that set (cov / kmer_count rebased), next to it on the device
            std::vector<DevContig> hd = job->h_contigs;
            for (size_t c = 0; c < n; ++c) {
                hd[c].cov = (const uint16_t*)(other + (job->chains[c].o_cov - job->sample_lo));
                hd[c].kmer_count = (const uint16_t*)(other + (job->chains[c].o_kcnt - job->sample_lo));
            }
            if (hipMemcpyAsync(d_other, hd.data(), sizeof(DevContig) * n, hipMemcpyHostToDevice, job->copy_stream) != hipSuccess ||
                hipStreamSynchronize(job->copy_stream) != hipSuccess) { r = PG_ERR_DEVICE; snprintf(e, sizeof(e), "descriptor upload failed"); }
            else job->h_contigs.swap(hd);
        }
        job->up_bytes[0] = 0; job->up_bytes[1] = bytes;
        job->upload_rc = r;
        job->upload_err = e;
    });
    return PG_OK;
}

extern "C" int pg_job_upload_end(pg_job* job, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->upload_pending) { set_err(err, errlen, "no upload in flight"); return PG_ERR_INVALID; }
    const double t0 = now_s();
    if (job->uploader.joinable()) job->uploader.join();
    job->upload_pending = false;
    job->host_s[1] = now_s() - t0;   // (what the caller waited: 0 when the upload hid behind the run)
    if (job->upload_rc != PG_OK) { set_err(err, errlen, "%s", job->upload_err.c_str()); return job->upload_rc; }
    // the freshly filled set becomes the current one: its descriptors sit in d_contigs_alt — swap the two descriptor arrays
    std::swap(job->d_contigs, job->d_contigs_alt);
    job->cur_samples = job->cur_samples == job->alt_samples ? job->arena + job->sample_lo : job->alt_samples;
    for (size_t c = 0; c < job->chains.size(); ++c) {
        job->chains[c].coverage.swap(job->next_coverage[c]);
        job->chains[c].d = job->h_contigs[c];
    }
    job->ran = false;
    return PG_OK;
}

// One sample's arrays written by a kernel of the count plan instead of an upload (pg_device.h: the seam to pg_kmers.hip).
extern "C" int pgi_job_fill_begin(pg_job* job, uint32_t sample, int device, uint32_t n_contigs, const uint32_t* n_variants,
                                  const uint32_t* const* kmer_off, void* stream, uint16_t** d_kmer_count, uint16_t** d_coverage,
                                  char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->cohort) { set_err(err, errlen, "not a cohort job"); return PG_ERR_INVALID; }
    if (job->upload_pending) { set_err(err, errlen, "an asynchronous upload is in flight: call pg_job_upload_end first"); return PG_ERR_INVALID; }
    if (job->device != device) { set_err(err, errlen, "the job is on device %d, the counter on device %d", job->device, device); return PG_ERR_INVALID; }
    if (sample >= job->n_samples) { set_err(err, errlen, "sample %u of %u", sample, job->n_samples); return PG_ERR_INVALID; }
    if (n_contigs != job->n_contigs) { set_err(err, errlen, "the plan has %u contigs, the job %u", n_contigs, job->n_contigs); return PG_ERR_INVALID; }
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const IndexHost& x = job->index[c];
        if (n_variants[c] != x.V || (x.V && memcmp(kmer_off[c], x.koff.data(), ((size_t)x.V + 1) * 4) != 0)) {
            set_err(err, errlen, "contig %u: variants or k-mers per variant of the plan differ from the resident job", c);
            return PG_ERR_INVALID;
        }
    }
    HIP_TRY(hipSetDevice(job->device));
    if (!job->ev_fill) HIP_TRY(hipEventCreateWithFlags(&job->ev_fill, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(job->ev_fill, job->stream));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, job->ev_fill, 0));
    // from here on the chains' arrays are being rewritten: whatever happens to the fill, the results of the last run no
    // longer belong to the inputs the job holds
    job->ran = false;
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const ChainHost& ch = job->chains[(size_t)sample * n_contigs + c];
        d_kmer_count[c] = (uint16_t*)(job->cur_samples + (ch.o_kcnt - job->sample_lo));
        d_coverage[c] = (uint16_t*)(job->cur_samples + (ch.o_cov - job->sample_lo));
    }
    return PG_OK;
}

extern "C" int pgi_job_fill_end(pg_job* job, uint32_t sample, uint32_t n_contigs, const uint16_t* const* coverage, void* stream,
                                char* err, size_t errlen) {
    HIP_TRY(hipEventRecord(job->ev_fill, (hipStream_t)stream));   // (the event _begin made)
    HIP_TRY(hipStreamWaitEvent(job->stream, job->ev_fill, 0));
    for (uint32_t c = 0; c < n_contigs; ++c) {
        const uint32_t V = job->index[c].V;
        if (V) job->chains[(size_t)sample * n_contigs + c].coverage.assign(coverage[c], coverage[c] + V);
    }
    job->ran = false;
    return PG_OK;
}

extern "C" int pg_job_fetch(pg_job* job, uint32_t ci, pg_contig_result* out, char* err, size_t errlen) {
    if (!job || !out || ci >= job->chains.size()) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    const double t0 = now_s();
    HIP_TRY(hipSetDevice(job->device));
    const ChainHost& c = job->chains[ci];
    const IndexHost& x = job->index[c.index];
    out->n_columns = c.n_cols_host;
    if (x.V == 0) return PG_OK;
    if (out->lik && x.n_lik) HIP_TRY(hipMemcpy(out->lik, c.d.lik, x.n_lik * sizeof(double), hipMemcpyDeviceToHost));
    if (out->lik_exp && x.n_lik) HIP_TRY(hipMemcpy(out->lik_exp, c.d.lik_exp, x.n_lik * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out->kept) HIP_TRY(hipMemcpy(out->kept, c.d.kept, x.V, hipMemcpyDeviceToHost));
    if (out->allele_present && x.sumA) HIP_TRY(hipMemcpy(out->allele_present, c.d.allele_present, x.sumA, hipMemcpyDeviceToHost));
    // reference src/hmm.cpp:94,106-109: set only when there is at least one column
    const bool fill = job->params.run_genotyping && c.n_cols_host > 0;
    // the Viterbi backtrace sets both at the COLUMN index (sic, reference src/hmm.cpp:164-165): entries [0, C)
    const size_t nvit = job->params.run_phasing ? c.n_cols_host : 0;
    if (out->n_kmers) {
        if (fill) memcpy(out->n_kmers, x.n_kmers.data(), (size_t)x.V * 2);
        else { memset(out->n_kmers, 0, (size_t)x.V * 2); memcpy(out->n_kmers, x.n_kmers.data(), nvit * 2); }
    }
    if (out->coverage) {
        if (fill) memcpy(out->coverage, c.coverage.data(), (size_t)x.V * 2);
        else { memset(out->coverage, 0, (size_t)x.V * 2); memcpy(out->coverage, c.coverage.data(), nvit * 2); }
    }
    if (job->params.run_phasing) {
        if (out->haplotype_1) HIP_TRY(hipMemcpy(out->haplotype_1, c.d.hap1, (size_t)x.V * 2, hipMemcpyDeviceToHost));
        if (out->haplotype_2) HIP_TRY(hipMemcpy(out->haplotype_2, c.d.hap2, (size_t)x.V * 2, hipMemcpyDeviceToHost));
    }
    job->host_s[3] += now_s() - t0;
    return PG_OK;
}

// All chains at once: the copies are queued on the job's stream and waited for once (24 chains x 6 blocking copies
// were 13 ms of the whole-genome job's 360 ms end-to-end time).
extern "C" int pg_job_fetch_all(pg_job* job, pg_contig_result* outs, char* err, size_t errlen) {
    if (!job || !outs) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    const double t0 = now_s();
    HIP_TRY(hipSetDevice(job->device));
    hipStream_t s = job->stream;
    for (size_t ci = 0; ci < job->chains.size(); ++ci) {
        const ChainHost& c = job->chains[ci];
        const IndexHost& x = job->index[c.index];
        pg_contig_result* out = &outs[ci];
        out->n_columns = c.n_cols_host;
        if (x.V == 0) continue;
        if (out->lik && x.n_lik) HIP_TRY(hipMemcpyAsync(out->lik, c.d.lik, x.n_lik * sizeof(double), hipMemcpyDeviceToHost, s));
        if (out->lik_exp && x.n_lik) HIP_TRY(hipMemcpyAsync(out->lik_exp, c.d.lik_exp, x.n_lik * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (out->kept) HIP_TRY(hipMemcpyAsync(out->kept, c.d.kept, x.V, hipMemcpyDeviceToHost, s));
        if (out->allele_present && x.sumA) HIP_TRY(hipMemcpyAsync(out->allele_present, c.d.allele_present, x.sumA, hipMemcpyDeviceToHost, s));
        if (job->params.run_phasing) {
            if (out->haplotype_1) HIP_TRY(hipMemcpyAsync(out->haplotype_1, c.d.hap1, (size_t)x.V * 2, hipMemcpyDeviceToHost, s));
            if (out->haplotype_2) HIP_TRY(hipMemcpyAsync(out->haplotype_2, c.d.hap2, (size_t)x.V * 2, hipMemcpyDeviceToHost, s));
        }
        // host-side meta data while the copies run (rules: pg_job_fetch)
        const bool fill = job->params.run_genotyping && c.n_cols_host > 0;
        const size_t nvit = job->params.run_phasing ? c.n_cols_host : 0;
        if (out->n_kmers) {
            if (fill) memcpy(out->n_kmers, x.n_kmers.data(), (size_t)x.V * 2);
            else { memset(out->n_kmers, 0, (size_t)x.V * 2); memcpy(out->n_kmers, x.n_kmers.data(), nvit * 2); }
        }
        if (out->coverage) {
            if (fill) memcpy(out->coverage, c.coverage.data(), (size_t)x.V * 2);
            else { memset(out->coverage, 0, (size_t)x.V * 2); memcpy(out->coverage, c.coverage.data(), nvit * 2); }
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    job->host_s[3] += now_s() - t0;
    return PG_OK;
}

// The inputs a job holds on the device, back on the host (the panel of a job made by pg_sampler_then_job never was there).
extern "C" int pg_job_panel_sizes(const pg_job* job, uint32_t ci, uint32_t* n_variants, uint32_t* n_paths, uint64_t* sum_kmers, uint64_t* sum_alleles) {
    if (!job || ci >= job->chains.size()) return PG_ERR_INVALID;
    const IndexHost& x = job->index[job->chains[ci].index];
    if (n_variants) *n_variants = x.V;
    if (n_paths) *n_paths = x.H;
    if (sum_kmers) *sum_kmers = x.sumK;
    if (sum_alleles) *sum_alleles = x.sumA;
    return PG_OK;
}
extern "C" int pg_job_fetch_panel(pg_job* job, uint32_t ci, uint32_t* kmer_off, uint16_t* kmer_count, uint32_t* allele_off, uint16_t* allele_id,
                                  uint8_t* allele_flags, uint16_t* allele_kmer_off, uint32_t* allele_kmer_mask, uint16_t* path_allele,
                                  char* err, size_t errlen) {
    if (!job || ci >= job->chains.size()) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    const ChainHost& c = job->chains[ci];
    const IndexHost& x = job->index[c.index];
    if (x.V == 0) return PG_OK;
    const unsigned char* A = job->arena;
    if (kmer_off) HIP_TRY(hipMemcpy(kmer_off, A + x.o_koff, ((size_t)x.V + 1) * 4, hipMemcpyDeviceToHost));
    if (kmer_count && x.sumK) HIP_TRY(hipMemcpy(kmer_count, job->cur_samples + (c.o_kcnt - job->sample_lo), (size_t)x.sumK * 2, hipMemcpyDeviceToHost));
    if (allele_off) HIP_TRY(hipMemcpy(allele_off, A + x.o_aoff, ((size_t)x.V + 1) * 4, hipMemcpyDeviceToHost));
    if (allele_id) HIP_TRY(hipMemcpy(allele_id, A + x.o_aid, (size_t)x.sumA * 2, hipMemcpyDeviceToHost));
    if (allele_flags) HIP_TRY(hipMemcpy(allele_flags, A + x.o_aflag, (size_t)x.sumA, hipMemcpyDeviceToHost));
    if (allele_kmer_off) HIP_TRY(hipMemcpy(allele_kmer_off, A + x.o_akoff, (size_t)x.sumA * 2, hipMemcpyDeviceToHost));
    if (allele_kmer_mask) HIP_TRY(hipMemcpy(allele_kmer_mask, A + x.o_akmask, (size_t)x.sumA * 4, hipMemcpyDeviceToHost));
    if (path_allele) HIP_TRY(hipMemcpy(path_allele, A + x.o_pa, (size_t)x.V * x.H * 2, hipMemcpyDeviceToHost));
    return PG_OK;
}

extern "C" int pg_job_device_results(pg_job* job, uint32_t ci, void** d_lik, uint64_t* n_lik, void** d_lik_exp, uint64_t* n_variants) {
    if (!job || ci >= job->chains.size()) return PG_ERR_INVALID;
    const ChainHost& c = job->chains[ci];
    const IndexHost& x = job->index[c.index];
    if (d_lik) *d_lik = c.d.lik;
    if (n_lik) *n_lik = x.n_lik;
    if (d_lik_exp) *d_lik_exp = c.d.lik_exp;
    if (n_variants) *n_variants = x.V;
    return PG_OK;
}

extern "C" int pg_job_packed_results(pg_job* job, void** d_lik, void** d_lik_exp, uint64_t* n_lik_total) {
    if (!job) return PG_ERR_INVALID;
    if (d_lik) *d_lik = job->d_lik;
    if (d_lik_exp) *d_lik_exp = job->d_likexp;
    if (n_lik_total) *n_lik_total = job->n_lik_total;
    return PG_OK;
}

extern "C" uint32_t pg_job_n_chains(const pg_job* job) { return job ? (uint32_t)job->chains.size() : 0; }

extern "C" int pg_job_host_seconds(const pg_job* job, double out4[4]) {
    if (!job || !out4) return PG_ERR_INVALID;
    for (int i = 0; i < 4; ++i) out4[i] = job->host_s[i];
    return PG_OK;
}
extern "C" int pg_job_upload_bytes(const pg_job* job, uint64_t out2[2]) {
    if (!job || !out2) return PG_ERR_INVALID;
    out2[0] = job->up_bytes[0]; out2[1] = job->up_bytes[1];
    return PG_OK;
}

extern "C" int pg_job_profile_counters(pg_job* job, uint32_t ci, uint64_t out64[64]) {
    if (!job || !out64 || ci >= job->chains.size()) return PG_ERR_INVALID;
    if (hipSetDevice(job->device) != hipSuccess) return PG_ERR_DEVICE;
    if (hipMemcpy(out64, job->chains[ci].d.prof, 64 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return PG_ERR_DEVICE;
    return PG_OK;
}

extern "C" int pg_job_kernel_ms(const pg_job* job, double ms[PG_N_KERNEL_CLASSES]) {
    if (!job || !ms) return PG_ERR_INVALID;
    for (int i = 0; i < PG_N_KERNEL_CLASSES; ++i) ms[i] = job->ms[i];
    return PG_OK;
}
extern "C" const char* pg_job_kernel_name(int cls) { return (cls >= 0 && cls < PG_N_KERNEL_CLASSES) ? kKernelNames[cls] : ""; }
extern "C" uint64_t pg_job_device_bytes(const pg_job* job) { return job ? job->arena_bytes : 0; }
extern "C" int pg_job_sweep_mode(const pg_job* job, uint32_t* chunk_cols) {
    if (!job) return PG_ERR_INVALID;
    if (chunk_cols) *chunk_cols = job->chunk_cols;
    return job->chunked ? 1 : 0;
}

extern "C" double pg_job_viterbi_ms(const pg_job* job) { return job ? job->vit_ms : 0.0; }

extern "C" double pg_job_index_ms(const pg_job* job) { return job ? job->index_ms : 0.0; }
extern "C" size_t pg_job_plan(const pg_job* job, char* out, size_t len) {
    if (!job) return 0;
    std::string t = job->plan_text;
    if (job->persist) {   // (what the runs so far really did: a run whose streams share a hardware queue takes a launch per chunk)
        char line[160];
        snprintf(line, sizeof(line), "  persistent phase 2: %u run(s), %u more fell back to a launch per chunk\n", job->persist_runs, job->persist_fallbacks);
        t += line;
    }
    if (out && len) { const size_t n = t.size() < len - 1 ? t.size() : len - 1; memcpy(out, t.data(), n); out[n] = 0; }
    return t.size() + 1;
}
// The segment arithmetic of the sparse phase 1 (pg_device.h: pg_sparse_*), as the kernels use it — for tests on the host.
extern "C" int pg_sparse_segment(uint32_t n_columns, uint32_t chunk_cols, uint32_t chunk, uint32_t role, uint32_t j, uint32_t out[3]) {
    if (role > 1u || chunk_cols == 0u || chunk_cols % PG_LEAN_SPARSE != 0u || j >= chunk_cols / PG_LEAN_SPARSE) return -1;
    const unsigned long long m = (unsigned long long)chunk * (chunk_cols / PG_LEAN_SPARSE) + j + 1u;
    if (m > pg_sparse_segments(n_columns, role)) return 0;
    const uint32_t ck = pg_sparse_checkpoint(n_columns, role, (uint32_t)m);
    if (out) { out[0] = ck; out[1] = role == 0u ? ck + 1u : ck - (PG_LEAN_SPARSE - 1u); out[2] = role == 0u ? ck + (PG_LEAN_SPARSE - 1u) : ck - 1u; }
    return 1;
}
// ... of phase 1 in pieces (pg_sparse_piece): piece `piece` of `piece_chunks` partner chunks; out = {lowest column, highest column}
extern "C" int pg_sparse_piece_range(uint32_t n_columns, uint32_t chunk_cols, uint32_t piece_chunks, uint32_t piece, uint32_t role, uint32_t out[2]) {
    if (role > 1u || chunk_cols == 0u || chunk_cols % PG_LEAN_SPARSE != 0u || piece_chunks == 0u || (unsigned long long)piece_chunks * chunk_cols > 0xFFFFFFFFull) return -1;
    uint32_t r[2];
    if (!pg_sparse_piece(n_columns, role, piece_chunks * chunk_cols, piece, r)) return 0;
    if (out) { out[0] = r[0]; out[1] = r[1]; }
    return 1;
}
// ... of the record ring of a sparse lean launch (pg_lean_ring_*): form 0 = phase 1 in one launch, 1 = piece `arg` of phase 1,
// 2 = chunk sweep `arg` of phase 3.  out = {column of the first step, steps, steps in front of the first group, number of the first
// step, step of a group that parks a block, step of a group that expands it}
extern "C" int pg_lean_ring_schedule(uint32_t n_columns, uint32_t chunk_cols, uint32_t piece_chunks, uint32_t role, uint32_t form, uint32_t arg, uint32_t out[6]) {
    if (role > 1u || form > 2u || chunk_cols == 0u || chunk_cols % PG_LEAN_SPARSE != 0u) return -1;
    if (form == 1u && (piece_chunks == 0u || piece_chunks > 0xFFFFu || arg > 0xFFFFu || (unsigned long long)piece_chunks * chunk_cols > 0xFFFFFFFFull)) return -1;
    uint32_t r[3];
    const uint32_t chunk = form == 0u ? 0u : (form == 1u ? (piece_chunks << 16 | arg) : arg);
    if (!pg_lean_ring_launch(n_columns, role, form == 2u ? 3u : 1u, chunk_cols, chunk, r)) return 0;
    if (out) { out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; out[3] = pg_lean_ring_first(r[2]); out[4] = PG_LEAN_RING_PARK; out[5] = PG_LEAN_RING_EXPAND; }
    return 1;
}
extern "C" uint32_t pg_lean_ring_image_offset(uint32_t record) { return pg_lean_ring_image(record); }
// ... of the preparation in parts (pg_prep_middle, pg_prep_middle_variants): the middle's columns and variants, [lo, hi) each
extern "C" int pg_prep_parts(uint32_t n_columns, uint32_t chunk_cols, uint32_t piece_chunks, uint32_t n_pieces, uint32_t early,
                             const uint32_t* col_variant, uint32_t n_variants, uint32_t out_cols[2], uint32_t out_vars[2]) {
    if (chunk_cols == 0u || chunk_cols % PG_LEAN_SPARSE != 0u || piece_chunks == 0u || (unsigned long long)piece_chunks * chunk_cols > 0xFFFFFFFFull) return -1;
    if (early == 0u || n_pieces == 0u || n_columns > n_variants) return -1;
    if (n_pieces < early + 1u) return 0;
    const uint32_t W = pg_prep_band(n_pieces, early, piece_chunks * chunk_cols);
    if (out_cols) pg_prep_middle(n_columns, W, out_cols);
    if (out_vars) {
        if (!col_variant && n_columns) return -1;
        pg_prep_middle_variants(col_variant, n_columns, n_variants, W, out_vars);
    }
    return 1;
}
extern "C" uint32_t pg_prep_part_member(uint32_t part, uint32_t lo, uint32_t hi, uint32_t n, uint32_t u) {
    if ((part != 1u && part != 2u) || lo > hi || hi > n) return n;
    return pg_prep_part_item(part, lo, hi, n, u);
}
// ... and of the sparse phase 2 (pg_sparse2_*): segment j of chunk `chunk`; out = {checkpoint, lowest column, highest column}
extern "C" int pg_sparse_chunk_segment(uint32_t n_columns, uint32_t chunk_cols, uint32_t chunk, uint32_t role, uint32_t j, uint32_t out[3]) {
    if (role > 1u || chunk_cols == 0u || chunk_cols % PG_LEAN_SPARSE != 0u || j >= chunk_cols / PG_LEAN_SPARSE) return -1;
    uint32_t seg[3];
    if (!pg_sparse2_segment(n_columns, role, (unsigned long long)chunk * (chunk_cols / PG_LEAN_SPARSE) + j, seg)) return 0;
    if (out) { out[0] = seg[0]; out[1] = seg[1]; out[2] = seg[2]; }
    return 1;
}
extern "C" int pg_sparse_chunk_stored_by_chain(uint32_t n_columns, uint32_t role, uint32_t column) {
    return role <= 1u && column < n_columns && pg_sparse2_stored(n_columns, role, column) ? 1 : 0;
}
extern "C" int pg_sparse_stored_by_chain(uint32_t n_columns, uint32_t role, uint32_t column) {
    return role <= 1u && column < n_columns && pg_sparse_stored(n_columns, role, column) ? 1 : 0;
}
extern "C" uint32_t pg_job_triangle_chains(const pg_job* job) {
    if (!job) return 0;
    uint32_t n = 0;
    for (const auto& ch : job->chains) n += ch.d.tri ? 1u : 0u;
    return n;
}

namespace {

// the body of the one-shot call for ONE chain: a job of its own (arena from / to the pool)
int genotype_single(const pg_contig_batch* batch, const pg_table* table, const pg_hmm_params* params, int device,
                    pg_contig_result* out, char* err, size_t errlen) {
    std::vector<ChainSpec> specs(1);
    specs[0] = {0, batch->kmer_count, batch->coverage};
    pg_job* job = nullptr;
    int rc = job_build(device, 1, batch, specs, 1, false, table, params, true, &job, err, errlen);
    if (rc != PG_OK) return rc;
    rc = pg_job_run(job, nullptr, err, errlen);
    if (rc == PG_OK) rc = pg_job_fetch(job, 0, out, err, errlen);
    pg_job_destroy(job);
    return rc;
}

// ---------------------------------------------------------------------------------------
//  Coalescing of concurrent one-shot calls.
//
//  The reference constructs one HMM per (contig x subset) on N thread-pool workers at a time
//  (src/commands.cpp:949-978, run_genotyping :155-185).  N one-shot jobs side by side would each bring their own
//  two streams (more streams than hardware queues: kernels of different jobs then queue behind each other's
//  half-chain kernels, which run for the whole phase), ~100 launches per job, and a k_post grid sized as if the job
//  had the chip to itself.  So calls that are in flight at the same time on the same device with the same table and
//  parameters are merged into ONE job — exactly the resident multi-chain job of pg_job_new — by whichever caller
//  arrives first (the leader); the others sleep until their results are in their buffers.  Chains of a job are
//  independent, so every caller gets bit for bit what it would have got alone.
//    * a leader launches when a job slot of the device is free (at most 2 merged jobs at a
//      time per device), every ANNOUNCED call has arrived (pg_hmm_announce: the C++ adapter announces at the top of
//      the HMM constructor, before it flattens its UniqueKmers — the leader then knows who is still coming; bounded by
//      PG_COALESCE_WAIT_MS = 250), and nobody new has joined for 300 us (only when other
//      callers have been seen at all: a single-threaded host never waits);
//    * if the merged job fails (one malformed batch, a device limit, no memory for the sum) the leader runs the
//      requests one by one, so every caller gets its own error code and message;
//    * PG_COALESCE=0 turns it off.
// ---------------------------------------------------------------------------------------
struct CoRequest {
    const pg_contig_batch* batch; pg_contig_result* out; char* err; size_t errlen;
    int rc = PG_OK; bool done = false;
};
struct CoBatch {
    int device; const pg_table* table; pg_hmm_params params;
    std::vector<CoRequest*> reqs;
    std::chrono::steady_clock::time_point last_arrival;
};
struct Coalescer {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::shared_ptr<CoBatch>> open;
    int callers_inside = 0;
    int announced[PG_MAX_DEVICES_HOST] = {0};
    int inflight[PG_MAX_DEVICES_HOST] = {0};
    std::chrono::steady_clock::time_point last_concurrency = std::chrono::steady_clock::time_point::min();
    uint64_t stat_batches = 0, stat_requests = 0, stat_largest = 0;
} g_co;

long env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? strtol(e, nullptr, 0) : dflt; }

bool same_params(const pg_hmm_params& a, const pg_hmm_params& b) {
    return a.effective_N == b.effective_N && a.recombrate == b.recombrate && (a.uniform != 0) == (b.uniform != 0) &&
           (a.run_genotyping != 0) == (b.run_genotyping != 0) && (a.run_phasing != 0) == (b.run_phasing != 0);
}

void run_merged(CoBatch& b) {
    const size_t n = b.reqs.size();
    pg_hmm_params prm = b.params;
    prm.reserved = 0;
    if (n > 1) {
        std::vector<pg_contig_batch> bs(n);
        std::vector<ChainSpec> specs(n);
        for (size_t i = 0; i < n; ++i) { bs[i] = *b.reqs[i]->batch; specs[i] = {(uint32_t)i, bs[i].kmer_count, bs[i].coverage}; }
        char err[512] = {0};
        pg_job* job = nullptr;
        int rc = job_build(b.device, (uint32_t)n, bs.data(), specs, 1, false, b.table, &prm, true, &job, err, sizeof(err));
        if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, sizeof(err));
        if (rc == PG_OK) {
            std::vector<pg_contig_result> outs(n);
            for (size_t i = 0; i < n; ++i) outs[i] = *b.reqs[i]->out;
            rc = pg_job_fetch_all(job, outs.data(), err, sizeof(err));
            for (size_t i = 0; i < n; ++i) b.reqs[i]->out->n_columns = outs[i].n_columns;
        }
        if (job) pg_job_destroy(job);
        if (rc == PG_OK) { for (CoRequest* r : b.reqs) r->rc = PG_OK; return; }
        // fall through: one by one, every caller its own verdict
    }
    for (CoRequest* r : b.reqs) r->rc = genotype_single(r->batch, b.table, &prm, b.device, r->out, r->err, r->errlen);
}

}  // namespace

extern "C" void pg_hmm_announce(int device) {
    if (device < 0 || device >= PG_MAX_DEVICES_HOST) return;
    std::lock_guard<std::mutex> lock(g_co.mu);
    g_co.announced[device] += 1;
}
extern "C" void pg_hmm_retract(int device) {
    if (device < 0 || device >= PG_MAX_DEVICES_HOST) return;
    std::lock_guard<std::mutex> lock(g_co.mu);
    if (g_co.announced[device] > 0) g_co.announced[device] -= 1;
    g_co.cv.notify_all();
}
extern "C" int pg_hmm_coalesce_stats(uint64_t out3[3]) {
    if (!out3) return PG_ERR_INVALID;
    std::lock_guard<std::mutex> lock(g_co.mu);
    out3[0] = g_co.stat_batches; out3[1] = g_co.stat_requests; out3[2] = g_co.stat_largest;
    return PG_OK;
}

extern "C" int pg_hmm_genotype_contig(const pg_contig_batch* batch, const pg_table* table, const pg_hmm_params* params,
                                      int device, pg_contig_result* out, char* err, size_t errlen) {
    if (!batch || !table || !params || !out) { set_err(err, errlen, "null argument"); return PG_ERR_INVALID; }
    using clock = std::chrono::steady_clock;
    static const bool enabled = env_long("PG_COALESCE", 1) != 0;
    static const long wait_ms = env_long("PG_COALESCE_WAIT_MS", 250);
    const long window_us = 300, max_inflight = 2, max_batch = 256;   // (measured settings)
    const bool announced = (params->reserved & PG_CALL_ANNOUNCED) != 0;
    if (!enabled || device < 0 || device >= PG_MAX_DEVICES_HOST) {
        if (announced) pg_hmm_retract(device);
        return genotype_single(batch, table, params, device, out, err, errlen);
    }
    CoRequest req{batch, out, err, errlen};
    std::shared_ptr<CoBatch> mine;
    {
        std::unique_lock<std::mutex> lk(g_co.mu);
        if (announced && g_co.announced[device] > 0) g_co.announced[device] -= 1;
        g_co.callers_inside += 1;
        if (g_co.callers_inside > 1) g_co.last_concurrency = clock::now();
        for (auto& ob : g_co.open)
            if (ob->device == device && ob->table == table && same_params(ob->params, *params) && (long)ob->reqs.size() < max_batch) {
                ob->reqs.push_back(&req);
                ob->last_arrival = clock::now();
                g_co.cv.notify_all();
                g_co.cv.wait(lk, [&] { return req.done; });
                g_co.callers_inside -= 1;
                return req.rc;
            }
        // leader of a new batch
        mine = std::make_shared<CoBatch>();
        mine->device = device; mine->table = table; mine->params = *params;
        mine->reqs.push_back(&req);
        mine->last_arrival = clock::now();
        g_co.open.push_back(mine);
        g_co.cv.notify_all();
        const clock::time_point hard = clock::now() + std::chrono::milliseconds(wait_ms);
        for (;;) {
            const clock::time_point now = clock::now();
            const bool concurrent = g_co.callers_inside > 1 || (g_co.last_concurrency != clock::time_point::min() &&
                                                                now - g_co.last_concurrency < std::chrono::seconds(2));
            const clock::time_point quiet_until = mine->last_arrival + std::chrono::microseconds(concurrent ? window_us : 0);
            const bool slot = g_co.inflight[device] < max_inflight;
            const bool coming = g_co.announced[device] > 0 && now < hard;
            const bool full = (long)mine->reqs.size() >= max_batch;
            if (slot && (full || (!coming && now >= quiet_until))) break;
            clock::time_point until = now + std::chrono::milliseconds(50);
            if (slot && !coming && quiet_until < until) until = quiet_until;
            if (coming && hard < until) until = hard;
            g_co.cv.wait_until(lk, until);
        }
        for (size_t i = 0; i < g_co.open.size(); ++i)
            if (g_co.open[i] == mine) { g_co.open.erase(g_co.open.begin() + (long)i); break; }
        g_co.inflight[device] += 1;
        g_co.stat_batches += 1; g_co.stat_requests += mine->reqs.size();
        if (mine->reqs.size() > g_co.stat_largest) g_co.stat_largest = mine->reqs.size();
    }
    try {
        run_merged(*mine);
    } catch (...) {   // (std::bad_alloc of the host-side vectors, ...): every caller of the batch gets an error — and is woken up below
        for (CoRequest* r : mine->reqs) {
            r->rc = PG_ERR_DEVICE;
            set_err(r->err, r->errlen, "merged one-shot job failed with a host exception");
        }
    }
    {
        std::lock_guard<std::mutex> lk(g_co.mu);
        g_co.inflight[device] -= 1;
        g_co.callers_inside -= 1;
        for (CoRequest* r : mine->reqs) r->done = true;
        g_co.cv.notify_all();
    }
    return req.rc;
}

// ---------------------------------------------------------------------------------------
//  unit-level entry points
// ---------------------------------------------------------------------------------------
extern "C" int pg_emission_table(const pg_contig_batch* batch, const pg_table* table, uint32_t v, int device,
                                 long double* out, int32_t* all_zeros_out, char* err, size_t errlen) {
    if (!batch || !table || !out || v >= batch->n_variants) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    pg_hmm_params p;
    memset(&p, 0, sizeof(p));
    p.effective_N = 25000.0L; p.recombrate = 1.26; p.run_genotyping = 1;
    pg_job* job = nullptr;
    int rc = pg_job_new(device, 1, batch, table, &p, &job, err, errlen);
    if (rc != PG_OK) return rc;
    const uint32_t A = batch->allele_off[v + 1] - batch->allele_off[v];
    double* dm = nullptr; int* de = nullptr;
    std::vector<double> m((size_t)A * A);
    std::vector<int> e((size_t)A * A);
    if (hipMalloc((void**)&dm, m.size() * 8 + 8) != hipSuccess || hipMalloc((void**)&de, e.size() * 4 + 8) != hipSuccess) {
        set_err(err, errlen, "hipMalloc failed"); rc = PG_ERR_NOMEM;
    } else {
        pgk_launch_emission_single(job->d_contigs, job->tab, v, dm, de, job->stream);
        if (hipStreamSynchronize(job->stream) != hipSuccess ||
            hipMemcpy(m.data(), dm, m.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(e.data(), de, e.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            set_err(err, errlen, "emission kernel failed: %s", hipGetErrorString(hipGetLastError())); rc = PG_ERR_DEVICE;
        }
    }
    if (dm) hipFree(dm);
    if (de) hipFree(de);
    pg_job_destroy(job);
    if (rc != PG_OK) return rc;
    bool all_zeros = true;  // reference src/emissionprobabilitycomputer.cpp:24,31-34
    for (size_t i = 0; i < m.size(); ++i) {
        out[i] = ldexpl((long double)m[i], e[i]);
        if (out[i] > 0) all_zeros = false;
    }
    if (all_zeros)
        for (size_t i = 0; i < m.size(); ++i) out[i] = 1.0L;
    if (all_zeros_out) *all_zeros_out = all_zeros ? 1 : 0;
    return PG_OK;
}

extern "C" int pg_transition_probs(uint64_t from_pos, uint64_t to_pos, double recombrate, uint32_t nr_paths, int uniform,
                                   long double effective_N, int device, double out3[3], char* err, size_t errlen) {
    if (!out3 || nr_paths == 0) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_err(err, errlen, "no HIP device available (no CPU fallback)"); return PG_ERR_DEVICE; }
    HIP_TRY(hipSetDevice(device));
    double* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 3 * sizeof(double)));
    const long double dist = (to_pos - from_pos) * 0.000004L * ((long double)recombrate) * effective_N;
    pgk_launch_transition_single((double)dist, nr_paths, uniform, d, nullptr);
    hipError_t he = hipMemcpy(out3, d, 3 * sizeof(double), hipMemcpyDeviceToHost);
    hipFree(d);
    if (he != hipSuccess) { set_err(err, errlen, "transition kernel failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
    return PG_OK;
}
