// pg_shim_calls.cpp — the C-ABI of the output columns formed from a job's finished bins (pg_calls.hip; DESIGN.md 4e .. 4e-3):
// the calls per variant, the calls per VCF record, the GL column per record and — from the last two — the bytes of the sample
// column (pg_record_text.hip, 4e-6).  Host code off the critical path.
//
// The three families differ in their descriptor type, in whether record plans and staging slots come along, and in what
// comes back; everything else is ONE path: the state a job keeps of a family (OutputFamily, pg_job.h), the opening checks
// and the timed launch of "form this family's output" (form_begin, timed_launch), the fetches (fetch_chain, fetch_all,
// fetch_packed, device_slice, each told the family by a Family row) and, for the unit entry points that take host arrays,
// the staging of one contig's bins (StagedBins).  A further column adds a Family row, its descriptors and its launch.
#include <hip/hip_runtime_api.h>

#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/pangenie_hmm.h"
#include "pg_calls.h"
#include "pg_device.h"
#include "pg_job.h"
#include "pg_launch.h"

using namespace pgj;

// ---------------------------------------------------------------------------------------
//  What the three families share
// ---------------------------------------------------------------------------------------
namespace {

// One output family as the shared code sees it.  The two flags are where the calls differ from the record families today;
// they are kept as they are, not repaired.
struct Family {
    OutputFamily pg_job::*state;
    size_t elem;            // bytes per element of the output (pg_call, pg_gl)
    const char* former;     // the entry point that forms the output, as the messages name it
    const char* elements;   // what the packed fetch calls the elements
    bool plans_once;        // calls: the shapes of a job never change, so the buffer is planned once and is ready (and its device
                            // pointers handed out) as soon as it exists; the record families rebuild when `dirty` and refuse until formed
    bool null_out_refused;  // calls: fetching one chain refuses a null `out` even for a chain without variants
};
static_assert(sizeof(pg_call) == 8, "pg_call is the 8-byte record k_calls stores");
static_assert(sizeof(pg_gl) == 4, "a GL value is 4 bytes");
const Family kCalls = {&pg_job::calls, sizeof(pg_call), "pg_job_calls", "calls", true, true};
const Family kRcalls = {&pg_job::rcalls, sizeof(pg_call), "pg_job_record_calls", "records", false, false};
const Family kRgl = {&pg_job::rgl, sizeof(pg_gl), "pg_job_record_gl", "GL values", false, false};

// ---- forming a family's output ----------------------------------------------------------------

// The genotype-quality thresholds, built once from log10l itself (pg_calls.h) and uploaded once per device.
struct GqTables {
    std::mutex mu;
    bool built = false, bad = false;
    uint64_t m[PG_GQ_STEPS];
    int32_t e[PG_GQ_STEPS];
    unsigned char* dev[PG_MAX_DEVICES_HOST] = {nullptr};
} g_gq;

}  // namespace

// (the caller has made `device` current; declared in pg_job.h: pg_shim_combine.cpp asks for the table too)
int pgj::gq_table_on(int device, const uint64_t** d_m, const int32_t** d_e, char* err, size_t errlen) {
    if (device < 0 || device >= PG_MAX_DEVICES_HOST) { set_err(err, errlen, "device %d out of range", device); return PG_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(g_gq.mu);
    if (!g_gq.built) {
        g_gq.bad = pgx_build_gq_table(g_gq.m, g_gq.e) != 0;
        g_gq.built = true;
    }
    if (g_gq.bad) { set_err(err, errlen, "the genotype-quality table could not be built: log10l is not monotone at a threshold"); return PG_ERR_INVALID; }
    constexpr size_t off_e = PG_GQ_STEPS * sizeof(uint64_t);
    if (!g_gq.dev[device]) {
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, off_e + PG_GQ_STEPS * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of the GQ table failed"); return PG_ERR_NOMEM; }
        if (hipMemcpy(d, g_gq.m, off_e, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d + off_e, g_gq.e, PG_GQ_STEPS * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(d);
            set_err(err, errlen, "upload of the GQ table failed");
            return PG_ERR_DEVICE;
        }
        g_gq.dev[device] = d;
    }
    *d_m = (const uint64_t*)g_gq.dev[device];
    *d_e = (const int32_t*)(g_gq.dev[device] + off_e);
    return PG_OK;
}

namespace {

// What every "form this family's output" opens with: the job has run a genotyping (`from_bins`: what the bins would have
// been for, for the message), its device is current, the GQ thresholds are on it where the family wants them (d_tm non-null)
// and the two events the families share exist.
int form_begin(pg_job* job, const char* from_bins, const uint64_t** d_tm, const int32_t** d_te, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->params.run_genotyping) { set_err(err, errlen, "the job does not run the genotyping: it has no bins to %s", from_bins); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    if (d_tm) {
        const int rc = gq_table_on(job->device, d_tm, d_te, err, errlen);
        if (rc != PG_OK) return rc;
    }
    if (!job->calls_events) {
        HIP_TRY(hipEventCreate(&job->ev_calls[0]));
        HIP_TRY(hipEventCreate(&job->ev_calls[1]));
        job->calls_events = true;
    }
    return PG_OK;
}

// launch(stream) between the two events on the job's stream, waited for; its time goes to the family, which is then formed
template <class Launch>
int timed_launch(pg_job* job, OutputFamily& f, Launch launch, char* err, size_t errlen) {
    hipStream_t s = job->stream;
    HIP_TRY(hipEventRecord(job->ev_calls[0], s));
    launch(s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev_calls[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, job->ev_calls[0], job->ev_calls[1]));
    f.ms = ms;
    f.formed = true;
    f.run = job->run_serial;
    return PG_OK;
}

// ---- fetching it ----------------------------------------------------------------------------------

int family_ready(pg_job* job, const Family& fam, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    const OutputFamily& f = job->*fam.state;
    if (fam.plans_once ? !f.d : (!f.formed || f.dirty)) { set_err(err, errlen, "%s has not been called", fam.former); return PG_ERR_INVALID; }
    return PG_OK;
}

// one chain's slice to the host
int fetch_chain(pg_job* job, const Family& fam, uint32_t ci, void* out, char* err, size_t errlen) {
    int rc = family_ready(job, fam, err, errlen);
    if (rc != PG_OK) return rc;
    if (ci >= job->chains.size() || (fam.null_out_refused && !out)) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const OutputFamily& f = job->*fam.state;
    const uint64_t n = f.first[ci + 1] - f.first[ci];
    if (!fam.null_out_refused) {   // (nothing to fetch: a null `out` will do)
        if (n == 0) return PG_OK;
        if (!out) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    }
    HIP_TRY(hipSetDevice(job->device));
    if (n) HIP_TRY(hipMemcpy(out, f.d + f.first[ci] * fam.elem, n * fam.elem, hipMemcpyDeviceToHost));
    return PG_OK;
}

// every chain's slice to its own buffer; a chain with nothing to fetch needs none
int fetch_all(pg_job* job, const Family& fam, void* const* outs, char* err, size_t errlen) {
    int rc = family_ready(job, fam, err, errlen);
    if (rc != PG_OK) return rc;
    if (!outs) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    const OutputFamily& f = job->*fam.state;
    for (size_t ci = 0; ci < job->chains.size(); ++ci) {
        const uint64_t n = f.first[ci + 1] - f.first[ci];
        if (n == 0) continue;
        if (!outs[ci]) { set_err(err, errlen, "no buffer for chain %zu", ci); return PG_ERR_INVALID; }
        HIP_TRY(hipMemcpyAsync(outs[ci], f.d + f.first[ci] * fam.elem, n * fam.elem, hipMemcpyDeviceToHost, job->stream));
    }
    HIP_TRY(hipStreamSynchronize(job->stream));
    return PG_OK;
}

// The packed fetch: the elements lie chain after chain on the device, so the whole of a family is one copy.
int fetch_packed(pg_job* job, const Family& fam, void* out, uint64_t n, char* err, size_t errlen) {
    int rc = family_ready(job, fam, err, errlen);
    if (rc != PG_OK) return rc;
    const OutputFamily& f = job->*fam.state;
    if (n != f.first.back()) { set_err(err, errlen, "the job holds %llu %s, not %llu", (unsigned long long)f.first.back(), fam.elements, (unsigned long long)n); return PG_ERR_INVALID; }
    if (n == 0) return PG_OK;
    if (!out) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    HIP_TRY(hipMemcpyAsync(out, f.d, n * fam.elem, hipMemcpyDeviceToHost, job->stream));
    HIP_TRY(hipStreamSynchronize(job->stream));
    return PG_OK;
}

// one chain's slice where it lies on the device
int device_slice(pg_job* job, const Family& fam, uint32_t ci, void** d_out, uint64_t* n) {
    if (!job || ci >= job->chains.size()) return PG_ERR_INVALID;
    const OutputFamily& f = job->*fam.state;
    if (!f.d || (!fam.plans_once && f.dirty)) return PG_ERR_INVALID;
    if (d_out) *d_out = f.d + f.first[ci] * fam.elem;
    if (n) *n = f.first[ci + 1] - f.first[ci];
    return PG_OK;
}

// ---- one contig's bins from host arrays, for the unit entry points ----------------------------------

// A region of the staged buffer: `bytes` of room at `at` (set by StagedBins::upload), filled from `src` if there is one.
struct Region {
    size_t bytes;
    const void* src;
    size_t at = 0;
    Region(size_t bytes_, const void* src_ = nullptr) : bytes(bytes_), src(src_) {}
};
using Regions = std::initializer_list<Region*>;

// One contig's host arrays, as the unit entry points receive them, as ONE device buffer with a DevContig in front.  The buffer
// goes with the object, on every path.  check(), then the caller's own checks, then select_device(), then upload().
struct StagedBins {
    uint32_t V;
    const uint32_t* allele_off;
    const uint16_t* allele_id;
    const uint8_t *kept, *allele_present;
    const double* lik;
    const int32_t* lik_exp;
    std::vector<uint64_t> goff;   // (check)
    unsigned char* d = nullptr;   // (upload)
    ~StagedBins() { if (d) hipFree(d); }

    // the index arrays are there and allele_off describes 1 .. PG_MAX_ALLELES_PER_VARIANT alleles per variant; forms geno_off
    int check() {
        if (V && (!allele_off || !allele_id || !kept || !allele_present || allele_off[0] != 0)) return PG_ERR_INVALID;
        goff.assign((size_t)V + 1, 0);
        for (uint32_t v = 0; v < V; ++v) {
            if (allele_off[v + 1] <= allele_off[v] || allele_off[v + 1] - allele_off[v] > PG_MAX_ALLELES_PER_VARIANT) return PG_ERR_INVALID;
            const uint64_t A = allele_off[v + 1] - allele_off[v];
            goff[v + 1] = goff[v] + A * (A + 1) / 2;
        }
        return PG_OK;
    }
    // the bins are there if the contig has any; `device` exists and is current
    int select_device(int device) const {
        if (goff[V] && (!lik || !lik_exp)) return PG_ERR_INVALID;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return PG_ERR_DEVICE; }
        if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return PG_ERR_DEVICE;
        return PG_OK;
    }
    // Lays out DevContig, `head`, the index arrays and geno_off, the bins, `tail`, every region at a 256-byte boundary, and
    // allocates.  place(d): the caller now knows every address, fixes the pointers of its descriptor and uploads what it uploads
    // itself (false: that failed).  Then the copies: DevContig, head, the index arrays and geno_off, tail, the bins.
    template <class Place>
    int upload(Regions head, Regions tail, Place place) {
        const size_t n_lik = goff[V], sumA = allele_off[V], V1 = (size_t)V + 1;
        DevContig dc;
        memset(&dc, 0, sizeof(dc));
        Region r_dc(sizeof(dc), &dc), r_aoff(V1 * 4, allele_off), r_aid(sumA * 2, allele_id), r_kept(V, kept), r_pres(sumA, allele_present),
            r_goff(V1 * 8, goff.data()), r_lik(n_lik * 8, lik), r_exp(n_lik * 4, lik_exp);
        const Regions front = {&r_dc}, index = {&r_aoff, &r_aid, &r_kept, &r_pres, &r_goff}, bins = {&r_lik, &r_exp};
        size_t o = 0;
        for (Regions list : {front, head, index, bins, tail})
            for (Region* r : list) { r->at = o; o += align_up(r->bytes + 8); }
        if (hipMalloc((void**)&d, o) != hipSuccess) { (void)hipGetLastError(); d = nullptr; return PG_ERR_NOMEM; }
        dc.V = V;
        dc.allele_off = (const uint32_t*)at(r_aoff);
        dc.allele_id = (const uint16_t*)at(r_aid);
        dc.kept = at(r_kept);
        dc.allele_present = at(r_pres);
        dc.geno_off = (const uint64_t*)at(r_goff);
        dc.lik = (double*)at(r_lik);
        dc.lik_exp = (int32_t*)at(r_exp);
        if (!place(d)) return PG_ERR_DEVICE;
        for (Regions list : {front, head, index, tail, bins})
            for (const Region* r : list)
                if (r->src && r->bytes && hipMemcpy(d + r->at, r->src, r->bytes, hipMemcpyHostToDevice) != hipSuccess) return PG_ERR_DEVICE;
        return PG_OK;
    }
    const DevContig* contig() const { return (const DevContig*)d; }   // (the first region)
    unsigned char* at(const Region& r) const { return d + r.at; }
    // after the caller's launch on the null stream: waits for it and copies `r` to the host
    int read_back(void* out, const Region& r) const {
        const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
                        (r.bytes == 0 || hipMemcpy(out, d + r.at, r.bytes, hipMemcpyDeviceToHost) == hipSuccess);
        return ok ? PG_OK : PG_ERR_DEVICE;
    }
};

}  // namespace

// ---------------------------------------------------------------------------------------
//  Genotype calls on the device (pg_calls.hip): GT and GQ per variant as 8-byte records.
// ---------------------------------------------------------------------------------------
namespace {

static_assert(PG_CALL_OK == PGX_CALL_OK && PG_CALL_NONE == PGX_CALL_NONE && PG_CALL_NOT_UNIQUE == PGX_CALL_NOT_UNIQUE &&
              PG_CALL_DEFERRED == PGX_CALL_DEFERRED, "the flags of the public header are the kernels' flags");

// descriptors and the list of wide variants of a set of chains: aoff(c) = allele_off of chain c (V + 1 entries), on the host
template <class AoffOf>
void plan_calls(uint32_t n_chains, const std::vector<uint32_t>& Vs, AoffOf aoff, std::vector<uint64_t>* first, std::vector<CallsDesc>* desc,
                std::vector<uint32_t>* wide, uint32_t* n_blocks) {
    const uint32_t per = pgk_calls_block();
    first->assign((size_t)n_chains + 1, 0);
    desc->clear();
    wide->clear();
    uint32_t blk = 0;
    for (uint32_t c = 0; c < n_chains; ++c) {
        const uint32_t V = Vs[c];
        (*first)[c + 1] = (*first)[c] + V;
        if (V == 0) continue;
        CallsDesc d;
        memset(&d, 0, sizeof(d));
        d.blk0 = blk; d.V = V; d.chain = c;
        const uint32_t* off = aoff(c);
        for (uint32_t v = 0; v < V; ++v)
            if (off[v + 1] - off[v] > PG_AMAX) { wide->push_back((uint32_t)desc->size()); wide->push_back(v); }
        desc->push_back(d);
        blk += (V + per - 1) / per;
    }
    *n_blocks = blk;
}

}  // namespace

extern "C" int pg_job_calls(pg_job* job, char* err, size_t errlen) {
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    int rc = form_begin(job, "call from", &d_tm, &d_te, err, errlen);
    if (rc != PG_OK) return rc;
    OutputFamily& f = job->calls;
    const uint32_t n = (uint32_t)job->chains.size();
    if (!f.d) {   // the shapes of a job never change: planned once (kCalls.plans_once)
        std::vector<uint32_t> Vs(n), wide;
        for (uint32_t c = 0; c < n; ++c) Vs[c] = job->index[job->chains[c].index].V;
        plan_calls(n, Vs, [&](uint32_t c) { return job->index[job->chains[c].index].aoff.data(); }, &f.first, &job->calls_desc, &wide, &f.blocks);
        f.wide = (uint32_t)(wide.size() / 2);
        f.o_desc = align_up((size_t)f.first[n] * sizeof(pg_call) + 8);
        f.o_wide = f.o_desc + align_up(job->calls_desc.size() * sizeof(CallsDesc) + 8);
        const size_t total = f.o_wide + align_up(wide.size() * sizeof(uint32_t) + 8);
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the calls failed", total); return PG_ERR_NOMEM; }
        for (CallsDesc& cd : job->calls_desc) cd.out = d + f.first[cd.chain] * sizeof(pg_call);
        hipError_t he = hipSuccess;
        if (!job->calls_desc.empty()) he = hipMemcpy(d + f.o_desc, job->calls_desc.data(), job->calls_desc.size() * sizeof(CallsDesc), hipMemcpyHostToDevice);
        if (he == hipSuccess && !wide.empty()) he = hipMemcpy(d + f.o_wide, wide.data(), wide.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (he != hipSuccess) { hipFree(d); set_err(err, errlen, "upload of the calls plan failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
        f.d = d;
    }
    return timed_launch(job, f, [&](hipStream_t s) {
        pgk_launch_calls(job->d_contigs, (const CallsDesc*)(f.d + f.o_desc), (uint32_t)job->calls_desc.size(), f.blocks, f.d + f.o_wide, f.wide, d_tm, d_te, s);
    }, err, errlen);
}

extern "C" int pg_job_fetch_calls(pg_job* job, uint32_t ci, pg_call* out, char* err, size_t errlen) { return fetch_chain(job, kCalls, ci, out, err, errlen); }
extern "C" int pg_job_fetch_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen) { return fetch_all(job, kCalls, (void* const*)outs, err, errlen); }
extern "C" int pg_job_device_calls(pg_job* job, uint32_t ci, void** d_calls, uint64_t* n) { return device_slice(job, kCalls, ci, d_calls, n); }
extern "C" double pg_job_calls_ms(const pg_job* job) { return job ? job->calls.ms : 0.0; }

// The unit entry point: host arrays in, records out, through the same two kernels.
extern "C" int pg_calls_from_bins(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id, const uint8_t* kept,
                                  const uint8_t* allele_present, const double* lik, const int32_t* lik_exp, pg_call* out) {
    if (n_variants == 0) return PG_OK;   // (before it looks at any pointer; the record variants check their plan first)
    StagedBins bins{n_variants, allele_off, allele_id, kept, allele_present, lik, lik_exp};
    int rc = bins.check();
    if (rc == PG_OK && !out) rc = PG_ERR_INVALID;
    if (rc == PG_OK) rc = bins.select_device(device);
    if (rc != PG_OK) return rc;
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    rc = gq_table_on(device, &d_tm, &d_te, nullptr, 0);
    if (rc != PG_OK) return rc;
    std::vector<uint64_t> first;
    std::vector<CallsDesc> desc;
    std::vector<uint32_t> wide, Vs(1, bins.V);
    uint32_t n_blocks = 0;
    plan_calls(1, Vs, [&](uint32_t) { return allele_off; }, &first, &desc, &wide, &n_blocks);
    Region r_desc(sizeof(CallsDesc), desc.data()), r_wide(wide.size() * 4, wide.data()), r_out((size_t)bins.V * sizeof(pg_call));
    rc = bins.upload({&r_desc, &r_wide}, {&r_out}, [&](unsigned char* d) { desc[0].out = d + r_out.at; return true; });
    if (rc != PG_OK) return rc;
    pgk_launch_calls(bins.contig(), (const CallsDesc*)bins.at(r_desc), 1, n_blocks, bins.at(r_wide), (uint32_t)(wide.size() / 2), d_tm, d_te, nullptr);
    return bins.read_back(out, r_out);
}

// ---------------------------------------------------------------------------------------
//  Genotype calls per VCF record (pg_calls.hip: k_rcalls / k_rcalls_wide, DESIGN.md 4e "Records").
// ---------------------------------------------------------------------------------------
namespace {

static_assert(PG_CALL_EMPTY == PGX_CALL_EMPTY, "the flag of the public header is the kernels' flag");

}  // namespace

// (declared in pg_job.h: pg_shim_combine.cpp forms the records of combined groups under the same plans)
namespace pgj {

// The checks that need the plan alone (everything but the allele ids), and the host copy the job keeps.
int check_record_plan(const pg_record_plan* p, uint32_t V, RecordPlanHost* h, char* err, size_t errlen) {
    if (!p) { set_err(err, errlen, "null record plan"); return PG_ERR_INVALID; }
    if (p->n_variants != V) { set_err(err, errlen, "the record plan has %u variants, the index contig %u", p->n_variants, V); return PG_ERR_INVALID; }
    RecordPlanHost r;
    r.set = true;
    r.V = V;
    if (V == 0) {
        if (p->n_records != 0) { set_err(err, errlen, "records without variants"); return PG_ERR_INVALID; }
        *h = std::move(r);
        return PG_OK;
    }
    if (!p->rec_off || !p->map_off || !p->map || !p->n_alleles || !p->vcf_off || !p->vcf_index) { set_err(err, errlen, "the record plan has null arrays"); return PG_ERR_INVALID; }
    if (p->rec_off[0] != 0 || p->map_off[0] != 0 || p->vcf_off[0] != 0) { set_err(err, errlen, "the record plan's offset arrays must start at 0"); return PG_ERR_INVALID; }
    for (uint32_t v = 0; v < V; ++v)
        if (p->rec_off[v + 1] <= p->rec_off[v]) { set_err(err, errlen, "rec_off does not grow at variant %u: every bubble has at least one record", v); return PG_ERR_INVALID; }
    const uint32_t R = p->rec_off[V];
    if (R != p->n_records || R >= 0x80000000u) { set_err(err, errlen, "n_records is %u, rec_off ends at %u", p->n_records, R); return PG_ERR_INVALID; }
    for (uint32_t q = 0; q < R; ++q) {
        if (p->map_off[q + 1] < p->map_off[q] || p->vcf_off[q + 1] < p->vcf_off[q]) { set_err(err, errlen, "map_off / vcf_off shrink at record %u", q); return PG_ERR_INVALID; }
        const uint32_t nA = p->n_alleles[q];
        if (nA == 0 || p->vcf_off[q + 1] - p->vcf_off[q] != nA) { set_err(err, errlen, "record %u: n_alleles is %u, vcf_off gives %u", q, nA, p->vcf_off[q + 1] - p->vcf_off[q]); return PG_ERR_INVALID; }
        if (nA > PG_MAX_ALLELES_PER_VARIANT) { set_err(err, errlen, "record %u has %u alleles: more than %d", q, nA, PG_MAX_ALLELES_PER_VARIANT); return PG_ERR_UNSUPPORTED; }
        for (uint32_t i = p->map_off[q]; i < p->map_off[q + 1]; ++i)
            if (p->map[i] >= nA) { set_err(err, errlen, "record %u: map entry %u is allele %u of %u", q, i - p->map_off[q], p->map[i], nA); return PG_ERR_INVALID; }
        uint16_t defined = 0;
        for (uint32_t a = 0; a < nA; ++a) {
            const uint16_t x = p->vcf_index[p->vcf_off[q] + a];
            if (x == 0xFFFFu && a > 0) continue;
            if (x != defined) { set_err(err, errlen, "record %u: vcf_index of allele %u is %u, not the running count of defined alleles %u", q, a, x, defined); return PG_ERR_INVALID; }
            ++defined;
        }
    }
    r.R = R;
    r.rec_off.assign(p->rec_off, p->rec_off + V + 1);
    r.map_off.assign(p->map_off, p->map_off + R + 1);
    r.vcf_off.assign(p->vcf_off, p->vcf_off + R + 1);
    r.map.assign(p->map, p->map + p->map_off[R]);
    r.vcf_index.assign(p->vcf_index, p->vcf_index + p->vcf_off[R]);
    r.rec_var.resize(R);
    for (uint32_t v = 0; v < V; ++v)
        for (uint32_t q = r.rec_off[v]; q < r.rec_off[v + 1]; ++q) {
            bool undef = false;
            for (uint32_t i = r.vcf_off[q]; i < r.vcf_off[q + 1]; ++i) undef = undef || r.vcf_index[i] == 0xFFFFu;
            r.rec_var[q] = v | (undef ? 0x80000000u : 0u);
        }
    *h = std::move(r);
    return PG_OK;
}

// every allele id of the contig's bubbles has an entry in the map of each of the bubble's records
int check_record_plan_ids(const RecordPlanHost& h, const uint32_t* allele_off, const uint16_t* allele_id, char* err, size_t errlen) {
    for (uint32_t v = 0; v < h.V; ++v)
        for (uint32_t q = h.rec_off[v]; q < h.rec_off[v + 1]; ++q) {
            const uint32_t len = h.map_off[q + 1] - h.map_off[q];
            for (uint32_t a = allele_off[v]; a < allele_off[v + 1]; ++a)
                if (allele_id[a] >= len) { set_err(err, errlen, "variant %u: allele id %u lies outside the map of record %u (%u entries)", v, allele_id[a], q, len); return PG_ERR_INVALID; }
        }
    return PG_OK;
}

size_t record_plan_device_bytes(const RecordPlanHost& h) {
    return align_up((size_t)h.R * 4 + 8) + 2 * align_up(((size_t)h.R + 1) * 4 + 8) + align_up(h.map.size() * 2 + 8) + align_up(h.vcf_index.size() * 2 + 8);
}
// copies the plan's arrays to d (record_plan_device_bytes of room) and points *dev at them
bool record_plan_upload(const RecordPlanHost& h, unsigned char* d, RecPlanDev* dev) {
    size_t o = 0;
    auto put = [&](const void* src, size_t bytes) -> const void* {
        unsigned char* at = d + o;
        o += align_up(bytes + 8);
        return (bytes == 0 || hipMemcpy(at, src, bytes, hipMemcpyHostToDevice) == hipSuccess) ? at : nullptr;
    };
    dev->rec_var = (const uint32_t*)put(h.rec_var.data(), (size_t)h.R * 4);
    dev->map_off = (const uint32_t*)put(h.map_off.data(), ((size_t)h.R + 1) * 4);
    dev->vcf_off = (const uint32_t*)put(h.vcf_off.data(), ((size_t)h.R + 1) * 4);
    dev->map = (const uint16_t*)put(h.map.data(), h.map.size() * 2);
    dev->vcf_index = (const uint16_t*)put(h.vcf_index.data(), h.vcf_index.size() * 2);
    return dev->rec_var && dev->map_off && dev->vcf_off && dev->map && dev->vcf_index;
}

// record r owns nd (nd + 1) / 2 values, nd its defined alleles
std::vector<uint64_t> record_gl_offsets(const RecordPlanHost& h) {
    std::vector<uint64_t> off((size_t)h.R + 1, 0);
    for (uint32_t q = 0; q < h.R; ++q) {
        uint64_t nd = 0;
        for (uint32_t i = h.vcf_off[q]; i < h.vcf_off[q + 1]; ++i) nd += h.vcf_index[i] != 0xFFFFu;
        off[q + 1] = off[q] + nd * (nd + 1) / 2;
    }
    return off;
}

// the plan of chain c's index contig, or nullptr
const RecordPlanHost* plan_of_chain(const pg_job* job, uint32_t c) {
    const uint32_t ix = job->chains[c].index;
    return ix < job->rplans.size() ? job->rplans[ix].get() : nullptr;
}

}  // namespace pgj

namespace {

// the checked plan on the job's device, ready to be referred to by index contigs
int record_plan_to_device(pg_job* job, RecordPlanHost&& h, RecordPlanRef* ref, char* err, size_t errlen) {
    HIP_TRY(hipSetDevice(job->device));
    if (h.R) {
        const size_t bytes = record_plan_device_bytes(h);
        if (hipMalloc((void**)&h.d, bytes) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the record plan failed", bytes); return PG_ERR_NOMEM; }
        if (!record_plan_upload(h, h.d, &h.dev)) { hipFree(h.d); set_err(err, errlen, "upload of the record plan failed"); return PG_ERR_DEVICE; }
    }
    *ref = record_plan_ref(std::move(h));
    if (job->rplans.size() != job->index.size()) job->rplans.resize(job->index.size());
    if (job->stream) HIP_TRY(hipStreamSynchronize(job->stream));   // (nothing reads the plans this one replaces any more)
    return PG_OK;
}

// a record family's rebuilt buffer takes the place of the one it had: nothing is formed in it yet
void adopt(OutputFamily& f, unsigned char* d, std::vector<uint64_t>&& first, const RcallsLaunch& L, size_t o_desc, size_t o_wide, size_t o_stage) {
    f.release();
    f.d = d;
    f.first = std::move(first);
    f.blocks = L.n_blocks; f.wide = (uint32_t)(L.wide.size() / 2);
    f.max_bins = L.max_bins; f.stride = L.stride; f.slots = L.n_slots;
    f.o_desc = o_desc; f.o_wide = o_wide; f.o_stage = o_stage;
    f.dirty = false;
    f.formed = false;
}

}  // namespace

// The id check on the device (k_rplan_ids): every allele id of every chain that has a plan, against the maps of its bubble's
// records.  `d_desc` = the RCallsDesc list of plan_rcalls on the device, `d_hit` = 8 bytes next to it.  On a hit the ids of
// that one chain come to the host and check_record_plan_ids forms the message.  (Declared in pg_job.h: pg_shim_phase.cpp
// asks for the same check in front of its first formation.)
int pgj::check_record_plan_ids_on_device(pg_job* job, const RCallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, unsigned char* d_hit, char* err,
                                         size_t errlen) {
    if (job->rplan_ids_ok || n_desc == 0 || n_blocks == 0) { job->rplan_ids_ok = true; return PG_OK; }
    hipStream_t s = job->stream;
    uint64_t hit = ~(uint64_t)0;
    HIP_TRY(hipMemcpyAsync(d_hit, &hit, sizeof(hit), hipMemcpyHostToDevice, s));
    pgk_launch_rplan_ids(job->d_contigs, d_desc, n_desc, n_blocks, d_hit, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&hit, d_hit, sizeof(hit), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hit == ~(uint64_t)0) { job->rplan_ids_ok = true; return PG_OK; }
    const uint32_t chain = (uint32_t)(hit >> 32);
    if (chain >= job->chains.size() || !plan_of_chain(job, chain)) { set_err(err, errlen, "the id check of the record plans answered chain %u", chain); return PG_ERR_DEVICE; }
    const IndexHost& x = job->index[job->chains[chain].index];
    std::vector<uint16_t> aid(x.sumA);
    HIP_TRY(hipMemcpy(aid.data(), job->arena + x.o_aid, (size_t)x.sumA * 2, hipMemcpyDeviceToHost));
    char text[256] = {0};
    const int rc = check_record_plan_ids(*plan_of_chain(job, chain), x.aoff.data(), aid.data(), text, sizeof(text));
    if (rc == PG_OK) { set_err(err, errlen, "chain %u, variant %u: an allele id lies outside a record's map", chain, (uint32_t)hit); return PG_ERR_INVALID; }
    set_err(err, errlen, "%s, in chain %u", text, chain);
    return rc;
}

extern "C" int pg_job_record_plan(pg_job* job, uint32_t ix, const pg_record_plan* plan, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (ix >= job->index.size()) { set_err(err, errlen, "index contig %u of %zu", ix, job->index.size()); return PG_ERR_INVALID; }
    RecordPlanHost h;
    int rc = check_record_plan(plan, job->index[ix].V, &h, err, errlen);
    if (rc != PG_OK) return rc;
    RecordPlanRef ref;
    rc = record_plan_to_device(job, std::move(h), &ref, err, errlen);
    if (rc != PG_OK) return rc;
    job->rplans[ix] = std::move(ref);   // (this index contig's reference alone: the members of a stride keep theirs)
    job->rlines.drop_prefix(ix);        // (the prefix of the lines had the old plan's records)
    job->plines.drop_prefix(ix);
    job->panellines.drop_prefix(ix);
    record_plans_changed(job);
    return PG_OK;
}

extern "C" int pg_job_record_plan_strided(pg_job* job, uint32_t contig, uint32_t n_contigs, const pg_record_plan* plan, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (n_contigs == 0 || contig >= n_contigs) { set_err(err, errlen, "contig %u of %u", contig, n_contigs); return PG_ERR_INVALID; }
    if (job->index.size() % n_contigs != 0) { set_err(err, errlen, "the job's %zu index contigs are no multiple of %u contigs", job->index.size(), n_contigs); return PG_ERR_INVALID; }
    if (!plan) { set_err(err, errlen, "null record plan"); return PG_ERR_INVALID; }
    for (size_t ix = contig; ix < job->index.size(); ix += n_contigs)
        if (job->index[ix].V != plan->n_variants) {
            set_err(err, errlen, "the record plan has %u variants, index contig %zu (member %zu of the stride) %u", plan->n_variants, ix, ix / n_contigs, job->index[ix].V);
            return PG_ERR_INVALID;
        }
    RecordPlanHost h;
    int rc = check_record_plan(plan, plan->n_variants, &h, err, errlen);
    if (rc != PG_OK) return rc;
    if (contig >= job->index.size()) return PG_OK;   // (a job without index contigs: no member)
    RecordPlanRef ref;
    rc = record_plan_to_device(job, std::move(h), &ref, err, errlen);
    if (rc != PG_OK) return rc;
    for (size_t ix = contig; ix < job->index.size(); ix += n_contigs) { job->rplans[ix] = ref; job->rlines.drop_prefix(ix); job->plines.drop_prefix(ix); job->panellines.drop_prefix(ix); }
    record_plans_changed(job);
    return PG_OK;
}

extern "C" int pg_job_record_calls(pg_job* job, char* err, size_t errlen) {
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    int rc = form_begin(job, "call from", &d_tm, &d_te, err, errlen);
    if (rc != PG_OK) return rc;
    OutputFamily& f = job->rcalls;
    const uint32_t n = (uint32_t)job->chains.size();
    if (f.dirty) {   // a plan or the index has changed: the descriptors and lists are made anew, the ids checked on the device
        RcallsLaunch L;
        plan_rcalls(n, [&](uint32_t c) { return plan_of_chain(job, c); }, [&](uint32_t c) { return job->index[job->chains[c].index].aoff.data(); }, pgk_calls_block(), &L);
        const size_t o_desc = align_up((size_t)L.first[n] * sizeof(pg_call) + 8);
        const size_t o_wide = o_desc + align_up(L.desc.size() * sizeof(RCallsDesc) + 8);
        const size_t o_stage = o_wide + align_up(L.wide.size() * sizeof(uint32_t) + 8);
        const size_t o_hit = o_stage + align_up((size_t)L.n_slots * L.stride * 16 + 8);
        const size_t total = o_hit + align_up(8);
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the record calls failed", total); return PG_ERR_NOMEM; }
        for (RCallsDesc& cd : L.desc) cd.out = d + L.first[cd.chain] * sizeof(pg_call);
        hipError_t he = hipSuccess;
        if (!L.desc.empty()) he = hipMemcpy(d + o_desc, L.desc.data(), L.desc.size() * sizeof(RCallsDesc), hipMemcpyHostToDevice);
        if (he == hipSuccess && !L.wide.empty()) he = hipMemcpy(d + o_wide, L.wide.data(), L.wide.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (he != hipSuccess) { hipFree(d); set_err(err, errlen, "upload of the record calls' lists failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
        rc = check_record_plan_ids_on_device(job, (const RCallsDesc*)(d + o_desc), (uint32_t)L.desc.size(), L.n_blocks, d + o_hit, err, errlen);
        if (rc != PG_OK) { hipFree(d); return rc; }
        adopt(f, d, std::move(L.first), L, o_desc, o_wide, o_stage);
        job->rcalls_desc = std::move(L.desc);
    }
    return timed_launch(job, f, [&](hipStream_t s) {
        pgk_launch_rcalls(job->d_contigs, (const RCallsDesc*)(f.d + f.o_desc), (uint32_t)job->rcalls_desc.size(), f.blocks, f.d + f.o_wide, f.wide,
                          f.d + f.o_stage, f.max_bins, f.stride, f.slots, d_tm, d_te, s);
    }, err, errlen);
}

extern "C" int pg_job_fetch_record_calls(pg_job* job, uint32_t ci, pg_call* out, char* err, size_t errlen) { return fetch_chain(job, kRcalls, ci, out, err, errlen); }
extern "C" int pg_job_fetch_record_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen) { return fetch_all(job, kRcalls, (void* const*)outs, err, errlen); }
extern "C" int pg_job_device_record_calls(pg_job* job, uint32_t ci, void** d_calls, uint64_t* n) { return device_slice(job, kRcalls, ci, d_calls, n); }
extern "C" double pg_job_record_calls_ms(const pg_job* job) { return job ? job->rcalls.ms : 0.0; }

namespace {

// What the record families' unit entry points open with: the bins' own checks, then the plan's — before V == 0 answers PG_OK
// (pg_calls_from_bins answers first) — then `out`, then the device.
int check_record_bins(StagedBins& bins, const uint32_t* allele_off, const uint16_t* allele_id, const pg_record_plan* plan, const void* out, int device,
                      RecordPlanHost* h) {
    int rc = bins.check();
    if (rc != PG_OK) return rc;
    rc = check_record_plan(plan, bins.V, h, nullptr, 0);
    if (rc == PG_OK && bins.V) rc = check_record_plan_ids(*h, allele_off, allele_id, nullptr, 0);
    if (rc != PG_OK || bins.V == 0) return rc;
    if (!out) return PG_ERR_INVALID;
    return bins.select_device(device);
}

}  // namespace

// The unit entry point: host arrays and a plan in, one record per VCF record out, through the same two kernels.
extern "C" int pg_record_calls_from_bins(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id, const uint8_t* kept,
                                         const uint8_t* allele_present, const double* lik, const int32_t* lik_exp, const pg_record_plan* plan,
                                         pg_call* out) {
    StagedBins bins{n_variants, allele_off, allele_id, kept, allele_present, lik, lik_exp};
    RecordPlanHost h;
    int rc = check_record_bins(bins, allele_off, allele_id, plan, out, device, &h);
    if (rc != PG_OK || n_variants == 0) return rc;
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    rc = gq_table_on(device, &d_tm, &d_te, nullptr, 0);
    if (rc != PG_OK) return rc;
    RcallsLaunch L;
    plan_rcalls(1, [&](uint32_t) -> const RecordPlanHost* { return &h; }, [&](uint32_t) { return allele_off; }, pgk_calls_block(), &L);
    Region r_desc(sizeof(RCallsDesc), L.desc.data()), r_wide(L.wide.size() * 4, L.wide.data()), r_plan(record_plan_device_bytes(h)),
        r_stage((size_t)L.n_slots * L.stride * 16), r_out((size_t)h.R * sizeof(pg_call));
    rc = bins.upload({&r_desc, &r_wide}, {&r_plan, &r_stage, &r_out}, [&](unsigned char* d) {
        L.desc[0].out = d + r_out.at;
        return record_plan_upload(h, d + r_plan.at, &L.desc[0].plan);
    });
    if (rc != PG_OK) return rc;
    pgk_launch_rcalls(bins.contig(), (const RCallsDesc*)bins.at(r_desc), 1, L.n_blocks, bins.at(r_wide), (uint32_t)(L.wide.size() / 2), bins.at(r_stage),
                      L.max_bins, L.stride, L.n_slots, d_tm, d_te, nullptr);
    return bins.read_back(out, r_out);
}

// ---------------------------------------------------------------------------------------
//  The GL column per VCF record (pg_calls.hip: k_rgl / k_rgl_wide / k_gl_values).
// ---------------------------------------------------------------------------------------
namespace {

RGlDesc rgl_desc_of(const RCallsDesc& c) {
    RGlDesc d;
    memset(&d, 0, sizeof(d));
    d.blk0 = c.blk0; d.R = c.R; d.chain = c.chain;
    d.plan = c.plan;
    return d;
}

}  // namespace

extern "C" int pg_record_gl_offsets(const pg_record_plan* plan, uint64_t* gl_off) {
    if (!plan || !gl_off) return PG_ERR_INVALID;
    RecordPlanHost h;
    const int rc = check_record_plan(plan, plan->n_variants, &h, nullptr, 0);
    if (rc != PG_OK) return rc;
    const std::vector<uint64_t> off = record_gl_offsets(h);
    memcpy(gl_off, off.data(), off.size() * sizeof(uint64_t));
    return PG_OK;
}

extern "C" int pg_gl_text(pg_gl value, char* buf, size_t len) { return pgx_gl_text(value, buf, len); }

extern "C" int pg_job_record_gl(pg_job* job, char* err, size_t errlen) {
    int rc = form_begin(job, "form likelihoods from", nullptr, nullptr, err, errlen);
    if (rc != PG_OK) return rc;
    OutputFamily& f = job->rgl;
    const uint32_t n = (uint32_t)job->chains.size();
    if (f.dirty) {   // a plan or the index has changed: the ids are checked, the offsets, descriptors and lists made anew
        // the offsets hang on the plan alone: one array per PLAN, whatever the number of index contigs that refer to it
        struct PlanOffsets { std::vector<uint64_t> gl_off; size_t at = 0; };
        std::map<const RecordPlanHost*, PlanOffsets> offs;
        for (const RecordPlanRef& p : job->rplans)
            if (p && p->R && !offs.count(p.get())) offs[p.get()].gl_off = record_gl_offsets(*p);
        RcallsLaunch L;
        plan_rcalls(n, [&](uint32_t c) { return plan_of_chain(job, c); }, [&](uint32_t c) { return job->index[job->chains[c].index].aoff.data(); }, pgk_calls_block(), &L);
        std::vector<uint64_t> first((size_t)n + 1, 0);
        for (uint32_t c = 0; c < n; ++c) {
            const auto o = offs.find(plan_of_chain(job, c));
            first[c + 1] = first[c] + (o != offs.end() ? o->second.gl_off.back() : 0);
        }
        size_t total = align_up((size_t)first[n] * sizeof(pg_gl) + 8);
        for (auto& kv : offs) {
            kv.second.at = total;
            total += align_up(kv.second.gl_off.size() * sizeof(uint64_t) + 8);
        }
        const size_t o_desc = total;
        const size_t o_wide = o_desc + align_up(L.desc.size() * sizeof(RGlDesc) + 8);
        const size_t o_stage = o_wide + align_up(L.wide.size() * sizeof(uint32_t) + 8);
        // (the id check reads the descriptors of the record calls: a copy of them and its word behind the staging slots; no room
        // for the copy once the ids have passed, so the buffer's size hangs on whether pg_job_record_calls came first)
        const size_t o_ids = o_stage + align_up((size_t)L.n_slots * L.stride * 16 + 8);
        const size_t o_hit = o_ids + align_up((job->rplan_ids_ok ? 0 : L.desc.size()) * sizeof(RCallsDesc) + 8);
        total = o_hit + align_up(8);
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the record GLs failed", total); return PG_ERR_NOMEM; }
        std::vector<RGlDesc> desc;
        for (const RCallsDesc& c : L.desc) {
            RGlDesc g = rgl_desc_of(c);
            g.out = d + first[c.chain] * sizeof(pg_gl);
            g.gl_off = (const uint64_t*)(d + offs[plan_of_chain(job, c.chain)].at);
            desc.push_back(g);
        }
        hipError_t he = hipSuccess;
        for (auto& kv : offs)
            if (he == hipSuccess) he = hipMemcpy(d + kv.second.at, kv.second.gl_off.data(), kv.second.gl_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (he == hipSuccess && !desc.empty()) he = hipMemcpy(d + o_desc, desc.data(), desc.size() * sizeof(RGlDesc), hipMemcpyHostToDevice);
        if (he == hipSuccess && !L.wide.empty()) he = hipMemcpy(d + o_wide, L.wide.data(), L.wide.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (he == hipSuccess && !job->rplan_ids_ok && !L.desc.empty()) he = hipMemcpy(d + o_ids, L.desc.data(), L.desc.size() * sizeof(RCallsDesc), hipMemcpyHostToDevice);
        if (he != hipSuccess) { hipFree(d); set_err(err, errlen, "upload of the record GLs' lists failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
        rc = check_record_plan_ids_on_device(job, (const RCallsDesc*)(d + o_ids), (uint32_t)L.desc.size(), L.n_blocks, d + o_hit, err, errlen);
        if (rc != PG_OK) { hipFree(d); return rc; }
        adopt(f, d, std::move(first), L, o_desc, o_wide, o_stage);
        job->rgl_desc = std::move(desc);
    }
    return timed_launch(job, f, [&](hipStream_t s) {
        pgk_launch_rgl(job->d_contigs, (const RGlDesc*)(f.d + f.o_desc), (uint32_t)job->rgl_desc.size(), f.blocks, f.d + f.o_wide, f.wide, f.d + f.o_stage,
                       f.max_bins, f.stride, f.slots, s);
    }, err, errlen);
}

extern "C" int pg_job_fetch_record_gl(pg_job* job, uint32_t ci, pg_gl* out, char* err, size_t errlen) { return fetch_chain(job, kRgl, ci, out, err, errlen); }
extern "C" int pg_job_fetch_record_gl_all(pg_job* job, pg_gl* const* outs, char* err, size_t errlen) { return fetch_all(job, kRgl, (void* const*)outs, err, errlen); }
extern "C" int pg_job_device_record_gl(pg_job* job, uint32_t ci, void** d_gl, uint64_t* n) { return device_slice(job, kRgl, ci, d_gl, n); }
extern "C" double pg_job_record_gl_ms(const pg_job* job) { return job ? job->rgl.ms : 0.0; }

// where every chain's records and values begin, for the packed fetches
extern "C" int pg_job_record_first(pg_job* job, uint64_t* calls_first, uint64_t* gl_first, char* err, size_t errlen) {
    if (!calls_first && !gl_first) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    int rc = calls_first ? family_ready(job, kRcalls, err, errlen) : PG_OK;
    if (rc == PG_OK && gl_first) rc = family_ready(job, kRgl, err, errlen);
    if (rc != PG_OK) return rc;
    if (calls_first) memcpy(calls_first, job->rcalls.first.data(), job->rcalls.first.size() * sizeof(uint64_t));
    if (gl_first) memcpy(gl_first, job->rgl.first.data(), job->rgl.first.size() * sizeof(uint64_t));
    return PG_OK;
}

extern "C" int pg_job_fetch_record_calls_packed(pg_job* job, pg_call* out, uint64_t n, char* err, size_t errlen) { return fetch_packed(job, kRcalls, out, n, err, errlen); }
extern "C" int pg_job_fetch_record_gl_packed(pg_job* job, pg_gl* out, uint64_t n, char* err, size_t errlen) { return fetch_packed(job, kRgl, out, n, err, errlen); }

// The unit entry point: host arrays and a plan in, the records' GL values out, through the same two kernels.
extern "C" int pg_record_gl_from_bins(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id, const uint8_t* kept,
                                      const uint8_t* allele_present, const double* lik, const int32_t* lik_exp, const pg_record_plan* plan, pg_gl* out) {
    StagedBins bins{n_variants, allele_off, allele_id, kept, allele_present, lik, lik_exp};
    RecordPlanHost h;
    int rc = check_record_bins(bins, allele_off, allele_id, plan, out, device, &h);
    if (rc != PG_OK || n_variants == 0) return rc;
    const std::vector<uint64_t> gl_off = record_gl_offsets(h);
    RcallsLaunch L;
    plan_rcalls(1, [&](uint32_t) -> const RecordPlanHost* { return &h; }, [&](uint32_t) { return allele_off; }, pgk_calls_block(), &L);
    RGlDesc gd;
    Region r_desc(sizeof(RGlDesc), &gd), r_wide(L.wide.size() * 4, L.wide.data()), r_plan(record_plan_device_bytes(h)),
        r_stage((size_t)L.n_slots * L.stride * 16), r_gloff(gl_off.size() * 8, gl_off.data()), r_out((size_t)gl_off.back() * sizeof(pg_gl));
    rc = bins.upload({&r_desc, &r_wide}, {&r_plan, &r_stage, &r_gloff, &r_out}, [&](unsigned char* d) {
        const bool ok = record_plan_upload(h, d + r_plan.at, &L.desc[0].plan);
        gd = rgl_desc_of(L.desc[0]);
        gd.out = d + r_out.at;
        gd.gl_off = (const uint64_t*)(d + r_gloff.at);
        return ok;
    });
    if (rc != PG_OK) return rc;
    pgk_launch_rgl(bins.contig(), (const RGlDesc*)bins.at(r_desc), 1, L.n_blocks, bins.at(r_wide), (uint32_t)(L.wide.size() / 2), bins.at(r_stage), L.max_bins,
                   L.stride, L.n_slots, nullptr);
    return bins.read_back(out, r_out);
}

// The unit entry point of the digits alone: out[i] = the GL of m[i] 2^e[i] by the device's own log10 / log1p.
extern "C" int pg_gl_from_values(int device, uint64_t n, const uint64_t* m, const int32_t* e, pg_gl* out) {
    if (n == 0) return PG_OK;
    if (!m || !e || !out || n > 0x7FFFFFFFull) return PG_ERR_INVALID;
    for (uint64_t i = 0; i < n; ++i)   // a pair is normalised, or zero with exponent 0
        if (m[i] == 0 ? e[i] != 0 : ((m[i] >> 63) == 0 || e[i] < -40000 || e[i] > 40000)) return PG_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return PG_ERR_DEVICE; }
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return PG_ERR_DEVICE;
    const size_t o_e = align_up(n * 8 + 8), o_out = o_e + align_up(n * 4 + 8), total = o_out + align_up(n * 4 + 8);
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); return PG_ERR_NOMEM; }
    bool ok = hipMemcpy(d, m, n * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d + o_e, e, n * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        pgk_launch_gl_values((const uint64_t*)d, (const int32_t*)(d + o_e), d + o_out, (uint32_t)n, nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
             hipMemcpy(out, d + o_out, n * sizeof(pg_gl), hipMemcpyDeviceToHost) == hipSuccess;
    }
    hipFree(d);
    return ok ? PG_OK : PG_ERR_DEVICE;
}

// ---------------------------------------------------------------------------------------
//  The record text: the bytes of the GT:GQ:GL:KC column (pg_record_text.hip).
// ---------------------------------------------------------------------------------------
namespace {

// Where the arrays of one launch lie in ONE buffer: the packed text (`cap` bytes), then the offsets, the scan's arrays, the
// descriptors and the wide list.
struct RTextLayout {
    size_t o_off, o_loc, o_wlen, o_bsum, o_bbase, o_desc, o_wide, total;
    RTextLayout(uint64_t cap, uint64_t R, uint32_t n_blocks, size_t n_desc, size_t n_wide) {
        o_off = align_up((size_t)cap + 16);
        o_loc = o_off + align_up(((size_t)R + 1) * 8 + 8);
        o_wlen = o_loc + align_up((size_t)R * 4 + 8);
        o_bsum = o_wlen + align_up(n_wide * 4 + 8);
        o_bbase = o_bsum + align_up((size_t)n_blocks * 4 + 8);
        o_desc = o_bbase + align_up(((size_t)n_blocks + 1) * 8 + 8);
        o_wide = o_desc + align_up(n_desc * sizeof(RTextDesc) + 8);
        total = o_wide + align_up(n_wide * 8 + 8);
    }
};

void rtext_launch(const DevContig* d_contigs, unsigned char* d, const RTextLayout& L, uint32_t n_desc, uint32_t n_blocks, uint32_t n_wide, uint64_t R,
                  uint64_t cap, hipEvent_t e0, hipEvent_t e1, hipStream_t s) {
    pgk_launch_rtext(d_contigs, (const RTextDesc*)(d + L.o_desc), n_desc, n_blocks, d + L.o_wide, n_wide, (uint32_t*)(d + L.o_loc), (uint32_t*)(d + L.o_wlen),
                     (uint32_t*)(d + L.o_bsum), (uint64_t*)(d + L.o_bbase), (uint64_t*)(d + L.o_off), R, (char*)d, cap, e0, e1, s);
}

bool family_current(const pg_job* job, const OutputFamily& f) { return f.formed && !f.dirty && f.run == job->run_serial; }

}  // namespace

extern "C" uint64_t pg_record_text_bound(uint64_t n_records, uint64_t n_gl_total) { return pgx_record_text_bound(n_records, n_gl_total); }

extern "C" int pg_job_record_text(pg_job* job, int ignore_imputed, char* err, size_t errlen) {
    int rc = form_begin(job, "form text from", nullptr, nullptr, err, errlen);
    if (rc != PG_OK) return rc;
    if (!family_current(job, job->rcalls) && (rc = pg_job_record_calls(job, err, errlen)) != PG_OK) return rc;
    if (!family_current(job, job->rgl) && (rc = pg_job_record_gl(job, err, errlen)) != PG_OK) return rc;
    RecordTextFamily& f = job->rtext;
    const uint32_t n = (uint32_t)job->chains.size();
    if (!f.events) {
        HIP_TRY(hipEventCreate(&f.ev_emit[0]));
        HIP_TRY(hipEventCreate(&f.ev_emit[1]));
        f.events = true;
    }
    if (f.dirty) {   // a plan or the index has changed: the two families above have been rebuilt, this one follows them
        if (job->rcalls_desc.size() != job->rgl_desc.size()) { set_err(err, errlen, "the record calls and the record GLs describe different chains"); return PG_ERR_INVALID; }
        const uint32_t per = pgk_rtext_block(), wide_above = pgk_rtext_wide_values();
        std::map<const RecordPlanHost*, std::vector<uint64_t>> offs;   // (one array per PLAN)
        std::vector<RTextDesc> desc;
        std::vector<uint32_t> wide;
        uint32_t blk = 0;
        for (size_t i = 0; i < job->rcalls_desc.size(); ++i) {
            const RCallsDesc& c = job->rcalls_desc[i];
            const RGlDesc& g = job->rgl_desc[i];
            if (c.chain != g.chain || c.R != g.R) { set_err(err, errlen, "the record calls and the record GLs describe different chains"); return PG_ERR_INVALID; }
            RTextDesc d;
            memset(&d, 0, sizeof(d));
            d.blk0 = blk; d.R = c.R; d.rec0 = job->rcalls.first[c.chain]; d.chain = c.chain;
            d.calls = c.out; d.gl = g.out; d.gl_off = g.gl_off; d.rec_var = c.plan.rec_var;
            const RecordPlanHost* h = plan_of_chain(job, c.chain);
            auto it = offs.find(h);
            if (it == offs.end()) it = offs.emplace(h, record_gl_offsets(*h)).first;
            const std::vector<uint64_t>& go = it->second;
            for (uint32_t q = 0; q < c.R; ++q)
                if (go[q + 1] - go[q] > wide_above) { wide.push_back((uint32_t)desc.size()); wide.push_back(q); }
            desc.push_back(d);
            blk += (c.R + per - 1) / per;
        }
        const uint64_t R = job->rcalls.first[n], cap = pgx_record_text_bound(R, job->rgl.first[n]);
        const RTextLayout L(cap, R, blk, desc.size(), wide.size() / 2);
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, L.total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the record text failed", L.total); return PG_ERR_NOMEM; }
        if (!wide.empty() && hipMemcpy(d + L.o_wide, wide.data(), wide.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(d);
            set_err(err, errlen, "upload of the record text's wide list failed");
            return PG_ERR_DEVICE;
        }
        f.OutputFamily::release();
        f.d = d;
        f.first = job->rcalls.first;
        f.desc = std::move(desc);
        f.blocks = blk; f.wide = (uint32_t)(wide.size() / 2);
        f.o_off = L.o_off; f.o_loc = L.o_loc; f.o_wlen = L.o_wlen; f.o_bsum = L.o_bsum; f.o_bbase = L.o_bbase; f.o_desc = L.o_desc; f.o_wide = L.o_wide;
        f.n_records = R; f.cap = cap;
        f.dirty = false;
        f.formed = false;
    }
    for (RTextDesc& d : f.desc) d.ignore_imputed = ignore_imputed ? 1u : 0u;
    const RTextLayout L(f.cap, f.n_records, f.blocks, f.desc.size(), f.wide);
    if (!f.desc.empty()) HIP_TRY(hipMemcpyAsync(f.d + L.o_desc, f.desc.data(), f.desc.size() * sizeof(RTextDesc), hipMemcpyHostToDevice, job->stream));
    f.formed = false;
    rc = timed_launch(job, f, [&](hipStream_t s) {
        rtext_launch(job->d_contigs, f.d, L, (uint32_t)f.desc.size(), f.blocks, f.wide, f.n_records, f.cap, f.ev_emit[0], f.ev_emit[1], s);
    }, err, errlen);
    if (rc != PG_OK) { f.formed = false; return rc; }
    f.formed = false;   // (until every chain's first byte is known)
    f.emit_ms = 0.0;
    f.text_first.assign((size_t)n + 1, 0);
    if (!f.desc.empty() && f.blocks) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, f.ev_emit[0], f.ev_emit[1]));
        f.emit_ms = ms;
        std::vector<uint64_t> bbase((size_t)f.blocks + 1);
        HIP_TRY(hipMemcpy(bbase.data(), f.d + L.o_bbase, bbase.size() * 8, hipMemcpyDeviceToHost));
        if (bbase.back() > f.cap) { set_err(err, errlen, "the record text takes %llu bytes, more than its bound %llu", (unsigned long long)bbase.back(), (unsigned long long)f.cap); return PG_ERR_DEVICE; }
        size_t i = 0;   // a chain begins a block: its first byte is that block's
        for (uint32_t c = 0; c < n; ++c) {
            f.text_first[c] = i < f.desc.size() ? bbase[f.desc[i].blk0] : bbase.back();
            if (i < f.desc.size() && f.desc[i].chain == c) ++i;
        }
        f.text_first[n] = bbase.back();
    }
    f.formed = true;
    f.serial += 1;
    return PG_OK;
}

extern "C" double pg_job_record_text_ms(const pg_job* job) { return job ? job->rtext.ms : 0.0; }
extern "C" double pg_job_record_text_emit_ms(const pg_job* job) { return job ? job->rtext.emit_ms : 0.0; }

// ---- what the two text families (the record text; the phased text of pg_shim_phase.cpp) share: declared in pg_job.h -------

int pgj::text_family_ready(pg_job* job, const TextKind& k, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (k.per_run && !job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    const RecordTextFamily& f = job->*k.text;
    if (!f.formed || f.dirty || (k.per_run && f.run != job->run_serial)) { set_err(err, errlen, "%s has not been called for this run and these plans", k.former); return PG_ERR_INVALID; }
    return PG_OK;
}

namespace {

// records [r0, r1) of a formed text family: their offsets less `minus` (or none) and their bytes, n_bytes of them
int text_family_fetch(pg_job* job, const RecordTextFamily& f, uint64_t r0, uint64_t r1, uint64_t b0, uint64_t b1, uint64_t minus, uint64_t* off, char* text,
                      uint64_t n_bytes, char* err, size_t errlen) {
    if (n_bytes != b1 - b0) { set_err(err, errlen, "the text holds %llu bytes, not %llu", (unsigned long long)(b1 - b0), (unsigned long long)n_bytes); return PG_ERR_INVALID; }
    if (n_bytes && !text) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    if (off) {
        if (f.n_records == 0) off[0] = 0;
        else HIP_TRY(hipMemcpyAsync(off, f.d + f.o_off + r0 * 8, (r1 - r0 + 1) * 8, hipMemcpyDeviceToHost, job->stream));
    }
    if (n_bytes) HIP_TRY(hipMemcpyAsync(text, f.d + b0, n_bytes, hipMemcpyDeviceToHost, job->stream));
    HIP_TRY(hipStreamSynchronize(job->stream));
    if (off && minus && f.n_records)
        for (uint64_t q = 0; q <= r1 - r0; ++q) off[q] -= minus;
    return PG_OK;
}

}  // namespace

int pgj::text_family_first(pg_job* job, const TextKind& k, uint64_t* text_first, char* err, size_t errlen) {
    int rc = text_family_ready(job, k, err, errlen);
    if (rc != PG_OK) return rc;
    if (!text_first) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const RecordTextFamily& f = job->*k.text;
    memcpy(text_first, f.text_first.data(), f.text_first.size() * sizeof(uint64_t));
    return PG_OK;
}

int pgj::text_family_fetch_chain(pg_job* job, const TextKind& k, uint32_t ci, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    int rc = text_family_ready(job, k, err, errlen);
    if (rc != PG_OK) return rc;
    if (ci >= job->chains.size()) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const RecordTextFamily& f = job->*k.text;
    return text_family_fetch(job, f, f.first[ci], f.first[ci + 1], f.text_first[ci], f.text_first[ci + 1], f.text_first[ci], off, text, n_bytes, err, errlen);
}

int pgj::text_family_fetch_packed(pg_job* job, const TextKind& k, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    int rc = text_family_ready(job, k, err, errlen);
    if (rc != PG_OK) return rc;
    const RecordTextFamily& f = job->*k.text;
    return text_family_fetch(job, f, 0, f.n_records, 0, f.text_first.back(), 0, off, text, n_bytes, err, errlen);
}

int pgj::text_family_device(pg_job* job, const TextKind& k, uint32_t ci, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes) {
    if (text_family_ready(job, k, nullptr, 0) != PG_OK || ci >= job->chains.size()) return PG_ERR_INVALID;
    const RecordTextFamily& f = job->*k.text;
    if (d_off) *d_off = f.d + f.o_off + f.first[ci] * 8;
    if (d_text) *d_text = f.d + f.text_first[ci];
    if (n_records) *n_records = f.first[ci + 1] - f.first[ci];
    if (n_bytes) *n_bytes = f.text_first[ci + 1] - f.text_first[ci];
    return PG_OK;
}

extern "C" int pg_job_record_text_first(pg_job* job, uint64_t* text_first, char* err, size_t errlen) { return text_family_first(job, kRecordText, text_first, err, errlen); }
extern "C" int pg_job_fetch_record_text(pg_job* job, uint32_t ci, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return text_family_fetch_chain(job, kRecordText, ci, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_fetch_record_text_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return text_family_fetch_packed(job, kRecordText, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_device_record_text(pg_job* job, uint32_t ci, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes) {
    return text_family_device(job, kRecordText, ci, d_off, d_text, n_records, n_bytes);
}

// The unit entry point: arbitrary fields in, the packed text and its offsets out, through the same kernels.
extern "C" int pg_record_text_from_fields(int device, uint64_t n_records, const pg_call* calls, const uint64_t* gl_off, const pg_gl* gl, const uint16_t* kc,
                                          const uint8_t* no_call, uint64_t* off, char* text, uint64_t cap) {
    if (!off || !gl_off || n_records >= 0x80000000ull) return PG_ERR_INVALID;
    if (n_records && (!calls || !kc)) return PG_ERR_INVALID;
    if (gl_off[0] != 0) return PG_ERR_INVALID;
    for (uint64_t q = 0; q < n_records; ++q)
        if (gl_off[q + 1] < gl_off[q]) return PG_ERR_INVALID;
    const uint64_t n_gl = gl_off[n_records];
    if ((n_gl && !gl) || cap < pgx_record_text_bound(n_records, n_gl) || (cap && !text)) return PG_ERR_INVALID;
    for (uint64_t q = 0; q < n_records; ++q)   // what the bound counts on: GT numbers up to 255, a GQ up to 10000
        if ((calls[q].flags & 0xFFu) == PG_CALL_OK && (calls[q].allele_1 > 255 || calls[q].allele_2 > 255 || calls[q].gq > PG_GQ_CERTAIN)) return PG_ERR_INVALID;
    if (n_records == 0) { off[0] = 0; return PG_OK; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return PG_ERR_DEVICE; }
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return PG_ERR_DEVICE;
    const uint32_t per = pgk_rtext_block(), wide_above = pgk_rtext_wide_values(), R = (uint32_t)n_records, n_blocks = (R + per - 1) / per;
    std::vector<uint32_t> wide;
    for (uint32_t q = 0; q < R; ++q)
        if (gl_off[q + 1] - gl_off[q] > wide_above) { wide.push_back(0); wide.push_back(q); }
    const uint64_t bound = pgx_record_text_bound(n_records, n_gl);
    const RTextLayout L(bound, R, n_blocks, 1, wide.size() / 2);
    // the inputs behind the launch's own arrays
    const size_t o_calls = L.total, o_gloff = o_calls + align_up((size_t)R * 8 + 8), o_gl = o_gloff + align_up(((size_t)R + 1) * 8 + 8),
                 o_kc = o_gl + align_up((size_t)n_gl * 4 + 8), o_nc = o_kc + align_up((size_t)R * 2 + 8), total = o_nc + align_up((size_t)R + 8);
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); return PG_ERR_NOMEM; }
    RTextDesc desc;
    memset(&desc, 0, sizeof(desc));
    desc.R = R;
    desc.calls = d + o_calls; desc.gl = d + o_gl; desc.gl_off = (const uint64_t*)(d + o_gloff); desc.kc = (const uint16_t*)(d + o_kc);
    desc.no_call = no_call ? d + o_nc : nullptr;
    bool ok = hipMemcpy(d + L.o_desc, &desc, sizeof(desc), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_calls, calls, (size_t)R * 8, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_gloff, gl_off, ((size_t)R + 1) * 8, hipMemcpyHostToDevice) == hipSuccess &&
              (n_gl == 0 || hipMemcpy(d + o_gl, gl, (size_t)n_gl * 4, hipMemcpyHostToDevice) == hipSuccess) &&
              hipMemcpy(d + o_kc, kc, (size_t)R * 2, hipMemcpyHostToDevice) == hipSuccess &&
              (!no_call || hipMemcpy(d + o_nc, no_call, R, hipMemcpyHostToDevice) == hipSuccess) &&
              (wide.empty() || hipMemcpy(d + L.o_wide, wide.data(), wide.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
    if (ok) {
        rtext_launch(nullptr, d, L, 1, n_blocks, (uint32_t)(wide.size() / 2), R, bound, nullptr, nullptr, nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
             hipMemcpy(off, d + L.o_off, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost) == hipSuccess && off[R] <= bound &&
             (off[R] == 0 || hipMemcpy(text, d, off[R], hipMemcpyDeviceToHost) == hipSuccess);
    }
    hipFree(d);
    return ok ? PG_OK : PG_ERR_DEVICE;
}
