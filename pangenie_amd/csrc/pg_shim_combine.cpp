// pg_shim_combine.cpp — the C-ABI of the path-subset flow (pg_combine.hip): a job's chains grouped per contig,
// the groups' bins added up on the device in the caller's order, the calls formed from the sums.  Host code off the critical path.
//
// A plan (pg_job_combine_plan) is the groups, the descriptors of the launches and ONE device buffer outside the arena for what
// they write; pg_job_combine and pg_job_combined_calls are a launch each over it and remember the run whose bins they read.
// The two unit entry points stage host arrays as DevContigs of their own and go through the same launchers.
//
// The records of the groups (pg_combine_records.hip) come last in this file: GT, GQ and the GL column per VCF
// record from the combined bins, under the record plans of pg_shim_calls.cpp — the plan of a group is that of its first
// chain's index contig.  Their state is pg_job::crec; their unit entry points stage one contig's combined bins and a plan.
#include <hip/hip_runtime_api.h>

#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../include/pangenie_hmm.h"
#include "pg_combine.h"
#include "pg_device.h"
#include "pg_job.h"
#include "pg_launch.h"

using namespace pgj;

namespace {

static_assert(sizeof(pg_combined_bin) == 16, "pg_combined_bin is the 16-byte record k_combine stores");
static_assert(sizeof(pg_call) == 8, "pg_call is the 8-byte record k_ccalls stores");

// descriptors and the wide list of a set of groups: V(g), aoff(g) = allele_off of group g's layout (V + 1 entries, on the host)
template <class VOf, class AoffOf>
void plan_groups(uint32_t n_groups, const std::vector<uint32_t>& group_off, VOf V_of, AoffOf aoff, std::vector<uint64_t>* bin_first,
                 std::vector<uint64_t>* var_first, std::vector<CombineDesc>* desc, std::vector<uint32_t>* wide, uint32_t* n_blocks) {
    const uint32_t per = pgk_combine_block();
    bin_first->assign((size_t)n_groups + 1, 0);
    var_first->assign((size_t)n_groups + 1, 0);
    desc->clear();
    wide->clear();
    uint32_t blk = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t V = V_of(g);
        const uint32_t* off = aoff(g);
        uint64_t bins = 0;
        for (uint32_t v = 0; v < V; ++v) {
            const uint64_t A = off[v + 1] - off[v];
            bins += A * (A + 1) / 2;
            if (A > PG_AMAX) { wide->push_back((uint32_t)desc->size()); wide->push_back(v); }
        }
        (*bin_first)[g + 1] = (*bin_first)[g] + bins;
        (*var_first)[g + 1] = (*var_first)[g] + V;
        if (V == 0) continue;
        CombineDesc d;
        memset(&d, 0, sizeof(d));
        d.blk0 = blk; d.V = V;
        d.first = group_off[g]; d.S = group_off[g + 1] - group_off[g];
        desc->push_back(d);
        blk += (V + per - 1) / per;
    }
    *n_blocks = blk;
}

// k_combine_check over the plan's pairs, on the job's stream; waits for the answer
int check_layout_on_device(pg_job* job, CombineState& c, unsigned char* d, char* err, size_t errlen) {
    if (c.pairs.empty()) { c.layout_ok = true; return PG_OK; }
    hipStream_t s = job->stream;
    uint32_t hit = 0;
    HIP_TRY(hipMemcpyAsync(d + c.o_hit, &hit, sizeof(hit), hipMemcpyHostToDevice, s));
    pgk_launch_combine_check(job->d_contigs, (const CombinePair*)(d + c.o_pairs), (uint32_t)c.pairs.size(), c.check_items, (uint32_t*)(d + c.o_hit), s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&hit, d + c.o_hit, sizeof(hit), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hit != 0) {
        const CombinePair& p = c.pairs[std::min<size_t>(hit - 1, c.pairs.size() - 1)];
        set_err(err, errlen, "chains %u and %u of one group differ in their alleles per variant or their allele ids", p.ref, p.member);
        return PG_ERR_INVALID;
    }
    c.layout_ok = true;
    return PG_OK;
}

// what pg_job_combine and pg_job_combined_calls open with
int combine_begin(pg_job* job, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->params.run_genotyping) { set_err(err, errlen, "the job does not run the genotyping: it has no bins to combine"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    if (!job->combine.planned) { set_err(err, errlen, "pg_job_combine_plan has not been called"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    CombineState& c = job->combine;
    if (!c.events) {
        HIP_TRY(hipEventCreate(&c.ev[0]));
        HIP_TRY(hipEventCreate(&c.ev[1]));
        c.events = true;
    }
    return PG_OK;
}

template <class Launch>
int timed(pg_job* job, Launch launch, double* ms_out, char* err, size_t errlen) {
    CombineState& c = job->combine;
    hipStream_t s = job->stream;
    HIP_TRY(hipEventRecord(c.ev[0], s));
    launch(s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    *ms_out = ms;
    return PG_OK;
}

// the combined bins (calls == false) or the combined calls of this run are there to be fetched
int combined_ready(pg_job* job, bool calls, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    const CombineState& c = job->combine;
    if (!c.planned || (calls ? c.calls_run : c.combined_run) != job->run_serial) {
        set_err(err, errlen, "%s has not been called for this run", calls ? "pg_job_combined_calls" : "pg_job_combine");
        return PG_ERR_INVALID;
    }
    return PG_OK;
}

int fetch_group(pg_job* job, bool calls, uint32_t g, void* out, char* err, size_t errlen) {
    int rc = combined_ready(job, calls, err, errlen);
    if (rc != PG_OK) return rc;
    const CombineState& c = job->combine;
    if (g + 1 >= c.group_off.size()) { set_err(err, errlen, "group %u of %zu", g, c.group_off.size() - 1); return PG_ERR_INVALID; }
    const std::vector<uint64_t>& first = calls ? c.var_first : c.bin_first;
    const size_t elem = calls ? sizeof(pg_call) : sizeof(pg_combined_bin);
    const uint64_t n = first[g + 1] - first[g];
    if (n == 0) return PG_OK;
    if (!out) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    HIP_TRY(hipMemcpy(out, c.d + (calls ? c.o_calls : 0) + first[g] * elem, n * elem, hipMemcpyDeviceToHost));
    return PG_OK;
}

int fetch_groups(pg_job* job, bool calls, void* const* outs, char* err, size_t errlen) {
    int rc = combined_ready(job, calls, err, errlen);
    if (rc != PG_OK) return rc;
    if (!outs) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const CombineState& c = job->combine;
    const std::vector<uint64_t>& first = calls ? c.var_first : c.bin_first;
    const size_t elem = calls ? sizeof(pg_call) : sizeof(pg_combined_bin);
    HIP_TRY(hipSetDevice(job->device));
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const uint64_t n = first[g + 1] - first[g];
        if (n == 0) continue;
        if (!outs[g]) { set_err(err, errlen, "no buffer for group %zu", g); return PG_ERR_INVALID; }
        HIP_TRY(hipMemcpyAsync(outs[g], c.d + (calls ? c.o_calls : 0) + first[g] * elem, n * elem, hipMemcpyDeviceToHost, job->stream));
    }
    HIP_TRY(hipStreamSynchronize(job->stream));
    return PG_OK;
}

int device_group(pg_job* job, bool calls, uint32_t g, void** d_out, uint64_t* n) {
    if (!job || !job->combine.planned || g + 1 >= job->combine.group_off.size()) return PG_ERR_INVALID;
    const CombineState& c = job->combine;
    if ((calls ? c.calls_run : c.combined_run) != job->run_serial || !job->ran) return PG_ERR_INVALID;
    const std::vector<uint64_t>& first = calls ? c.var_first : c.bin_first;
    const size_t elem = calls ? sizeof(pg_call) : sizeof(pg_combined_bin);
    if (d_out) *d_out = c.d + (calls ? c.o_calls : 0) + first[g] * elem;
    if (n) *n = first[g + 1] - first[g];
    return PG_OK;
}

}  // namespace

extern "C" int pg_job_combine_plan(pg_job* job, uint32_t n_groups, const uint32_t* group_off, const uint32_t* chains, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->params.run_genotyping) { set_err(err, errlen, "the job does not run the genotyping: it has no bins to combine"); return PG_ERR_INVALID; }
    if (n_groups == 0 || !group_off || !chains) { set_err(err, errlen, "a combine plan needs at least one group"); return PG_ERR_INVALID; }
    if (group_off[0] != 0) { set_err(err, errlen, "group_off must start at 0"); return PG_ERR_INVALID; }
    const size_t n_chains = job->chains.size();
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (group_off[g + 1] <= group_off[g]) { set_err(err, errlen, "group %u is empty", g); return PG_ERR_INVALID; }
        if ((size_t)group_off[g + 1] > n_chains) { set_err(err, errlen, "the groups list more chains than the job's %zu", n_chains); return PG_ERR_INVALID; }
    }
    CombineState c;
    c.group_off.assign(group_off, group_off + n_groups + 1);
    c.members.assign(chains, chains + group_off[n_groups]);
    std::vector<char> seen(n_chains, 0);
    for (uint32_t ch : c.members) {
        if (ch >= n_chains) { set_err(err, errlen, "chain %u of %zu", ch, n_chains); return PG_ERR_INVALID; }
        if (seen[ch]) { set_err(err, errlen, "chain %u is listed twice", ch); return PG_ERR_INVALID; }
        seen[ch] = 1;
    }
    // what the host knows of the layouts: variants, alleles per variant; the allele ids are the device's (k_combine_check)
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t ref = c.members[c.group_off[g]];
        const IndexHost& x0 = job->index[job->chains[ref].index];
        if (x0.V && x0.aoff.size() != (size_t)x0.V + 1) { set_err(err, errlen, "chain %u: the job does not keep its alleles per variant", ref); return PG_ERR_UNSUPPORTED; }
        for (uint32_t k = c.group_off[g] + 1; k < c.group_off[g + 1]; ++k) {
            const uint32_t ch = c.members[k];
            if (job->chains[ch].index == job->chains[ref].index) continue;
            const IndexHost& x = job->index[job->chains[ch].index];
            if (x.V != x0.V) { set_err(err, errlen, "group %u: chain %u has %u variants, chain %u has %u", g, ref, x0.V, ch, x.V); return PG_ERR_INVALID; }
            if (x.V && x.aoff.size() != (size_t)x.V + 1) { set_err(err, errlen, "chain %u: the job does not keep its alleles per variant", ch); return PG_ERR_UNSUPPORTED; }
            for (uint32_t v = 0; v <= x.V && x.V; ++v)
                if (x.aoff[v] != x0.aoff[v]) {
                    set_err(err, errlen, "group %u: chains %u and %u differ in their alleles per variant (variant %u)", g, ref, ch, v ? v - 1 : 0);
                    return PG_ERR_INVALID;
                }
            if (x.V == 0) continue;
            CombinePair p;
            p.ref = ref; p.member = ch; p.V = x.V; p.sumA = x.sumA;
            c.pairs.push_back(p);
            c.check_items = std::max(c.check_items, std::max(x.V + 1, x.sumA));
        }
    }
    std::vector<uint32_t> wide;
    plan_groups(n_groups, c.group_off, [&](uint32_t g) { return job->index[job->chains[c.members[c.group_off[g]]].index].V; },
                [&](uint32_t g) { return job->index[job->chains[c.members[c.group_off[g]]].index].aoff.data(); }, &c.bin_first, &c.var_first, &c.desc, &wide,
                &c.blocks);
    c.wide = (uint32_t)(wide.size() / 2);
    c.o_calls = align_up((size_t)c.bin_first[n_groups] * sizeof(pg_combined_bin) + 8);
    c.o_desc = c.o_calls + align_up((size_t)c.var_first[n_groups] * sizeof(pg_call) + 8);
    c.o_members = c.o_desc + align_up(c.desc.size() * sizeof(CombineDesc) + 8);
    c.o_wide = c.o_members + align_up(c.members.size() * sizeof(uint32_t) + 8);
    c.o_pairs = c.o_wide + align_up(wide.size() * sizeof(uint32_t) + 8);
    c.o_hit = c.o_pairs + align_up(c.pairs.size() * sizeof(CombinePair) + 8);
    const size_t total = c.o_hit + align_up(8);
    HIP_TRY(hipSetDevice(job->device));
    join_late_threads(job);   // (a pipelined first upload still copying: the check reads what it writes)
    if (job->stream2) HIP_TRY(hipStreamSynchronize(job->stream2));
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the combined bins failed", total); return PG_ERR_NOMEM; }
    {
        size_t gi = 0;
        for (uint32_t g = 0; g < n_groups; ++g) {
            if (c.var_first[g + 1] == c.var_first[g]) continue;
            c.desc[gi].bins = d + c.bin_first[g] * sizeof(pg_combined_bin);
            c.desc[gi].calls = d + c.o_calls + c.var_first[g] * sizeof(pg_call);
            ++gi;
        }
    }
    hipError_t he = hipSuccess;
    if (!c.desc.empty()) he = hipMemcpy(d + c.o_desc, c.desc.data(), c.desc.size() * sizeof(CombineDesc), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d + c.o_members, c.members.data(), c.members.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (he == hipSuccess && !wide.empty()) he = hipMemcpy(d + c.o_wide, wide.data(), wide.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (he == hipSuccess && !c.pairs.empty()) he = hipMemcpy(d + c.o_pairs, c.pairs.data(), c.pairs.size() * sizeof(CombinePair), hipMemcpyHostToDevice);
    if (he != hipSuccess) { hipFree(d); set_err(err, errlen, "upload of the combine plan failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
    const int rc = check_layout_on_device(job, c, d, err, errlen);
    if (rc != PG_OK) { hipFree(d); return rc; }
    // the new plan takes the place of the one the job had: nothing is combined in it yet
    if (job->stream) HIP_TRY(hipStreamSynchronize(job->stream));
    CombineState& mine = job->combine;
    if (mine.d) hipFree(mine.d);
    c.events = mine.events;
    c.ev[0] = mine.ev[0];
    c.ev[1] = mine.ev[1];
    c.d = d;
    c.planned = true;
    mine = std::move(c);
    job->crec.dirty = true;   // (the records of the groups: new groups, new bins)
    return PG_OK;
}

extern "C" int pg_job_combine(pg_job* job, char* err, size_t errlen) {
    int rc = combine_begin(job, err, errlen);
    if (rc != PG_OK) return rc;
    CombineState& c = job->combine;
    if (!c.layout_ok) {   // the index was uploaded anew: the layouts are compared before anything is combined
        rc = check_layout_on_device(job, c, c.d, err, errlen);
        if (rc != PG_OK) return rc;
    }
    rc = timed(job, [&](hipStream_t s) {
        pgk_launch_combine(job->d_contigs, (const CombineDesc*)(c.d + c.o_desc), (uint32_t)c.desc.size(), c.blocks, (const uint32_t*)(c.d + c.o_members),
                           c.d + c.o_wide, c.wide, s);
    }, &c.ms, err, errlen);
    if (rc == PG_OK) {
        c.combined_run = job->run_serial;
        ++job->combine_serial;   // (what was formed from the bins before is no longer this combine's)
    }
    return rc;
}

extern "C" int pg_job_combined_calls(pg_job* job, char* err, size_t errlen) {
    int rc = combine_begin(job, err, errlen);
    if (rc != PG_OK) return rc;
    CombineState& c = job->combine;
    if (c.combined_run != job->run_serial) { set_err(err, errlen, "pg_job_combine has not been called for this run"); return PG_ERR_INVALID; }
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    rc = gq_table_on(job->device, &d_tm, &d_te, err, errlen);
    if (rc != PG_OK) return rc;
    rc = timed(job, [&](hipStream_t s) {
        pgk_launch_ccalls(job->d_contigs, (const CombineDesc*)(c.d + c.o_desc), (uint32_t)c.desc.size(), c.blocks, (const uint32_t*)(c.d + c.o_members),
                          c.d + c.o_wide, c.wide, d_tm, d_te, s);
    }, &c.calls_ms, err, errlen);
    if (rc == PG_OK) c.calls_run = job->run_serial;
    return rc;
}

extern "C" int pg_job_fetch_combined(pg_job* job, uint32_t group, pg_combined_bin* out, char* err, size_t errlen) { return fetch_group(job, false, group, out, err, errlen); }
extern "C" int pg_job_fetch_combined_all(pg_job* job, pg_combined_bin* const* outs, char* err, size_t errlen) { return fetch_groups(job, false, (void* const*)outs, err, errlen); }
extern "C" int pg_job_device_combined(pg_job* job, uint32_t group, void** d_bins, uint64_t* n) { return device_group(job, false, group, d_bins, n); }
extern "C" int pg_job_fetch_combined_calls(pg_job* job, uint32_t group, pg_call* out, char* err, size_t errlen) { return fetch_group(job, true, group, out, err, errlen); }
extern "C" int pg_job_fetch_combined_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen) { return fetch_groups(job, true, (void* const*)outs, err, errlen); }
extern "C" int pg_job_device_combined_calls(pg_job* job, uint32_t group, void** d_calls, uint64_t* n) { return device_group(job, true, group, d_calls, n); }
extern "C" uint32_t pg_job_n_groups(const pg_job* job) { return job && job->combine.planned ? (uint32_t)(job->combine.group_off.size() - 1) : 0; }
extern "C" double pg_job_combine_ms(const pg_job* job) { return job ? job->combine.ms : 0.0; }
extern "C" double pg_job_combined_calls_ms(const pg_job* job) { return job ? job->combine.calls_ms : 0.0; }

// ---------------------------------------------------------------------------------------
//  The unit entry points: host arrays in, through the same launchers.
// ---------------------------------------------------------------------------------------
namespace {

// One device buffer filled region after region, every region at a 256-byte boundary; freed with the object.
struct Staged {
    struct Part { size_t at, bytes; const void* src; };
    std::vector<Part> parts;
    size_t total = 0;
    unsigned char* d = nullptr;
    ~Staged() { if (d) hipFree(d); }
    size_t add(size_t bytes, const void* src = nullptr) {
        parts.push_back({total, bytes, src});
        total += align_up(bytes + 8);
        return parts.size() - 1;
    }
    int alloc() {
        if (hipMalloc((void**)&d, total ? total : 8) != hipSuccess) { (void)hipGetLastError(); d = nullptr; return PG_ERR_NOMEM; }
        return PG_OK;
    }
    unsigned char* at(size_t part) const { return d + parts[part].at; }
    int copy_in() const {
        for (const Part& p : parts)
            if (p.src && p.bytes && hipMemcpy(d + p.at, p.src, p.bytes, hipMemcpyHostToDevice) != hipSuccess) return PG_ERR_DEVICE;
        return PG_OK;
    }
    int read_back(void* out, size_t part) const {
        const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
                        (parts[part].bytes == 0 || hipMemcpy(out, d + parts[part].at, parts[part].bytes, hipMemcpyDeviceToHost) == hipSuccess);
        return ok ? PG_OK : PG_ERR_DEVICE;
    }
};

// allele_off describes 1 .. PG_MAX_ALLELES_PER_VARIANT alleles per variant; forms geno_off
int layout_check(uint32_t V, const uint32_t* allele_off, std::vector<uint64_t>* goff) {
    if (!allele_off || allele_off[0] != 0) return PG_ERR_INVALID;
    goff->assign((size_t)V + 1, 0);
    for (uint32_t v = 0; v < V; ++v) {
        if (allele_off[v + 1] <= allele_off[v] || allele_off[v + 1] - allele_off[v] > PG_MAX_ALLELES_PER_VARIANT) return PG_ERR_INVALID;
        const uint64_t A = allele_off[v + 1] - allele_off[v];
        (*goff)[v + 1] = (*goff)[v] + A * (A + 1) / 2;
    }
    return PG_OK;
}

// a bin is a pg_combined_bin: zero, or normalised; deferred and absent bins carry no value
bool combined_bins_ok(const pg_combined_bin* bins, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const pg_combined_bin& b = bins[i];
        const bool value_ok = b.m == 0 ? b.e == 0 : ((b.m >> 63) != 0 && b.e > -40000 && b.e < 40000);
        if (!value_ok || (b.flags & ~(PG_COMBINED_PRESENT | PG_COMBINED_DEFERRED)) || (b.flags != PG_COMBINED_PRESENT && b.m != 0) ||
            b.flags == PG_COMBINED_DEFERRED)
            return false;
    }
    return true;
}

int select_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return PG_ERR_DEVICE; }
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return PG_ERR_DEVICE;
    return PG_OK;
}

}  // namespace

extern "C" int pg_combine_bins(int device, uint32_t n_variants, const uint32_t* allele_off, uint32_t n_chains, const uint8_t* const* kept,
                               const uint8_t* const* allele_present, const double* const* lik, const int32_t* const* lik_exp, pg_combined_bin* out) {
    if (n_variants == 0) return PG_OK;
    if (n_chains == 0 || !kept || !allele_present || !lik || !lik_exp || !out) return PG_ERR_INVALID;
    std::vector<uint64_t> goff;
    int rc = layout_check(n_variants, allele_off, &goff);
    if (rc != PG_OK) return rc;
    for (uint32_t s = 0; s < n_chains; ++s)
        if (!kept[s] || !allele_present[s] || !lik[s] || !lik_exp[s]) return PG_ERR_INVALID;
    rc = select_device(device);
    if (rc != PG_OK) return rc;
    const size_t V1 = (size_t)n_variants + 1, sumA = allele_off[n_variants], n_lik = goff[n_variants];
    std::vector<uint32_t> group_off = {0, n_chains}, members(n_chains), wide;
    for (uint32_t s = 0; s < n_chains; ++s) members[s] = s;
    std::vector<uint64_t> bin_first, var_first;
    std::vector<CombineDesc> desc;
    uint32_t n_blocks = 0;
    plan_groups(1, group_off, [&](uint32_t) { return n_variants; }, [&](uint32_t) { return allele_off; }, &bin_first, &var_first, &desc, &wide, &n_blocks);
    std::vector<DevContig> dcs(n_chains);
    memset(dcs.data(), 0, dcs.size() * sizeof(DevContig));
    Staged st;
    const size_t p_dc = st.add(dcs.size() * sizeof(DevContig), dcs.data()), p_desc = st.add(sizeof(CombineDesc), desc.data()),
                 p_mem = st.add(members.size() * 4, members.data()), p_wide = st.add(wide.size() * 4, wide.data()), p_aoff = st.add(V1 * 4, allele_off),
                 p_goff = st.add(V1 * 8, goff.data());
    std::vector<size_t> p_kept(n_chains), p_pres(n_chains), p_lik(n_chains), p_exp(n_chains);
    for (uint32_t s = 0; s < n_chains; ++s) {
        p_kept[s] = st.add(n_variants, kept[s]);
        p_pres[s] = st.add(sumA, allele_present[s]);
        p_lik[s] = st.add(n_lik * 8, lik[s]);
        p_exp[s] = st.add(n_lik * 4, lik_exp[s]);
    }
    const size_t p_out = st.add(n_lik * sizeof(pg_combined_bin));
    rc = st.alloc();
    if (rc != PG_OK) return rc;
    for (uint32_t s = 0; s < n_chains; ++s) {
        DevContig& dc = dcs[s];
        dc.V = n_variants;
        dc.allele_off = (const uint32_t*)st.at(p_aoff);
        dc.geno_off = (const uint64_t*)st.at(p_goff);
        dc.kept = st.at(p_kept[s]);
        dc.allele_present = st.at(p_pres[s]);
        dc.lik = (double*)st.at(p_lik[s]);
        dc.lik_exp = (int32_t*)st.at(p_exp[s]);
    }
    desc[0].bins = st.at(p_out);
    rc = st.copy_in();
    if (rc != PG_OK) return rc;
    pgk_launch_combine((const DevContig*)st.at(p_dc), (const CombineDesc*)st.at(p_desc), 1, n_blocks, (const uint32_t*)st.at(p_mem), st.at(p_wide),
                       (uint32_t)(wide.size() / 2), nullptr);
    return st.read_back(out, p_out);
}

extern "C" int pg_calls_from_combined(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id, const pg_combined_bin* bins,
                                      pg_call* out) {
    if (n_variants == 0) return PG_OK;
    if (!allele_id || !bins || !out) return PG_ERR_INVALID;
    std::vector<uint64_t> goff;
    int rc = layout_check(n_variants, allele_off, &goff);
    if (rc != PG_OK) return rc;
    const size_t V1 = (size_t)n_variants + 1, sumA = allele_off[n_variants], n_lik = goff[n_variants];
    if (!combined_bins_ok(bins, n_lik)) return PG_ERR_INVALID;
    rc = select_device(device);
    if (rc != PG_OK) return rc;
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    rc = gq_table_on(device, &d_tm, &d_te, nullptr, 0);
    if (rc != PG_OK) return rc;
    std::vector<uint32_t> group_off = {0, 1}, members = {0}, wide;
    std::vector<uint64_t> bin_first, var_first;
    std::vector<CombineDesc> desc;
    uint32_t n_blocks = 0;
    plan_groups(1, group_off, [&](uint32_t) { return n_variants; }, [&](uint32_t) { return allele_off; }, &bin_first, &var_first, &desc, &wide, &n_blocks);
    DevContig dc;
    memset(&dc, 0, sizeof(dc));
    Staged st;
    const size_t p_dc = st.add(sizeof(dc), &dc), p_desc = st.add(sizeof(CombineDesc), desc.data()), p_mem = st.add(4, members.data()),
                 p_wide = st.add(wide.size() * 4, wide.data()), p_aoff = st.add(V1 * 4, allele_off), p_aid = st.add(sumA * 2, allele_id),
                 p_goff = st.add(V1 * 8, goff.data()), p_bins = st.add(n_lik * sizeof(pg_combined_bin), bins), p_out = st.add((size_t)n_variants * sizeof(pg_call));
    rc = st.alloc();
    if (rc != PG_OK) return rc;
    dc.V = n_variants;
    dc.allele_off = (const uint32_t*)st.at(p_aoff);
    dc.allele_id = (const uint16_t*)st.at(p_aid);
    dc.geno_off = (const uint64_t*)st.at(p_goff);
    desc[0].bins = st.at(p_bins);
    desc[0].calls = st.at(p_out);
    rc = st.copy_in();
    if (rc != PG_OK) return rc;
    pgk_launch_ccalls((const DevContig*)st.at(p_dc), (const CombineDesc*)st.at(p_desc), 1, n_blocks, (const uint32_t*)st.at(p_mem), st.at(p_wide),
                      (uint32_t)(wide.size() / 2), d_tm, d_te, nullptr);
    return st.read_back(out, p_out);
}

// ---------------------------------------------------------------------------------------
//  GT, GQ and GL per VCF record of the combined groups (pg_combine_records.hip).
// ---------------------------------------------------------------------------------------
namespace {

static_assert(sizeof(pg_gl) == 4, "a GL value is 4 bytes");

// the plan of group g: that of its first chain's index contig, or nullptr
const RecordPlanHost* plan_of_group(const pg_job* job, uint32_t g) {
    const CombineState& c = job->combine;
    const uint32_t ix = job->chains[c.members[c.group_off[g]]].index;
    return ix < job->rplans.size() ? job->rplans[ix].get() : nullptr;
}

// one array of GL offsets per PLAN, whatever the number of groups under it
struct PlanOffsets { std::vector<uint64_t> gl_off; size_t at = 0; };

// the buffer of pg_job::crec for the plans, the groups and the combined bins as they are
int crec_rebuild(pg_job* job, char* err, size_t errlen) {
    const CombineState& c = job->combine;
    CombinedRecordsState& k = job->crec;
    const uint32_t n = (uint32_t)(c.group_off.size() - 1);
    RcallsLaunch L;
    plan_rcalls(n, [&](uint32_t g) { return plan_of_group(job, g); },
                [&](uint32_t g) { return job->index[job->chains[c.members[c.group_off[g]]].index].aoff.data(); }, pgk_combined_records_block(), &L);
    std::map<const RecordPlanHost*, PlanOffsets> offs;
    std::vector<uint64_t> gl_first((size_t)n + 1, 0);
    for (uint32_t g = 0; g < n; ++g) {
        const RecordPlanHost* h = plan_of_group(job, g);
        if (h && h->R && !offs.count(h)) offs[h].gl_off = record_gl_offsets(*h);
        gl_first[g + 1] = gl_first[g] + (h && h->R ? offs[h].gl_off.back() : 0);
    }
    const size_t o_gl = align_up((size_t)L.first[n] * sizeof(pg_call) + 8);
    size_t total = o_gl + align_up((size_t)gl_first[n] * sizeof(pg_gl) + 8);
    for (auto& kv : offs) {
        kv.second.at = total;
        total += align_up(kv.second.gl_off.size() * sizeof(uint64_t) + 8);
    }
    const size_t o_desc = total;
    const size_t o_wide = o_desc + align_up(L.desc.size() * sizeof(CRecDesc) + 8);
    const size_t o_stage = o_wide + align_up(L.wide.size() * sizeof(uint32_t) + 8);
    const size_t o_hit = o_stage + align_up((size_t)L.n_slots * L.stride * 16 + 8);
    total = o_hit + align_up(8);
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the records of the combined groups failed", total); return PG_ERR_NOMEM; }
    std::vector<CRecDesc> desc;
    for (const RCallsDesc& rc : L.desc) {   // (plan_rcalls' "chain" is the group)
        const uint32_t g = rc.chain;
        CRecDesc cd;
        memset(&cd, 0, sizeof(cd));
        cd.blk0 = rc.blk0; cd.R = rc.R;
        cd.chain = c.members[c.group_off[g]]; cd.group = g;
        cd.bins = c.d + c.bin_first[g] * sizeof(pg_combined_bin);
        cd.calls = d + L.first[g] * sizeof(pg_call);
        cd.gl = d + o_gl + gl_first[g] * sizeof(pg_gl);
        cd.gl_off = (const uint64_t*)(d + offs[plan_of_group(job, g)].at);
        cd.plan = rc.plan;
        desc.push_back(cd);
    }
    hipError_t he = hipSuccess;
    for (auto& kv : offs)
        if (he == hipSuccess) he = hipMemcpy(d + kv.second.at, kv.second.gl_off.data(), kv.second.gl_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (he == hipSuccess && !desc.empty()) he = hipMemcpy(d + o_desc, desc.data(), desc.size() * sizeof(CRecDesc), hipMemcpyHostToDevice);
    if (he == hipSuccess && !L.wide.empty()) he = hipMemcpy(d + o_wide, L.wide.data(), L.wide.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (he != hipSuccess) { hipFree(d); set_err(err, errlen, "upload of the combined groups' record lists failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
    if (job->stream) HIP_TRY(hipStreamSynchronize(job->stream));   // (nothing reads the buffer this one replaces any more)
    k.release();
    k.d = d;
    k.rec_first = std::move(L.first);
    k.gl_first = std::move(gl_first);
    k.desc = std::move(desc);
    k.o_gl = o_gl; k.o_desc = o_desc; k.o_wide = o_wide; k.o_stage = o_stage; k.o_hit = o_hit;
    k.blocks = L.n_blocks; k.wide = (uint32_t)(L.wide.size() / 2);
    k.max_bins = L.max_bins; k.stride = L.stride; k.slots = L.n_slots;
    k.dirty = false;
    k.ids_serial = k.calls_serial = k.gl_serial = 0;
    return PG_OK;
}

// k_crplan_ids over the groups' descriptors, on the job's stream; waits for the answer
int crec_check_ids(pg_job* job, char* err, size_t errlen) {
    CombinedRecordsState& k = job->crec;
    if (!k.desc.empty() && k.blocks) {
        hipStream_t s = job->stream;
        uint64_t hit = ~(uint64_t)0;
        HIP_TRY(hipMemcpyAsync(k.d + k.o_hit, &hit, sizeof(hit), hipMemcpyHostToDevice, s));
        pgk_launch_crplan_ids(job->d_contigs, (const CRecDesc*)(k.d + k.o_desc), (uint32_t)k.desc.size(), k.blocks, k.d + k.o_hit, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&hit, k.d + k.o_hit, sizeof(hit), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (hit != ~(uint64_t)0) {
            set_err(err, errlen, "group %u, variant %u: an allele id lies outside the map of one of the variant's records (the plan of the group's first chain)",
                    (uint32_t)(hit >> 32), (uint32_t)hit);
            return PG_ERR_INVALID;
        }
    }
    k.ids_serial = job->combine_serial;
    return PG_OK;
}

// what the two formations open with: the combined bins of this run are there, a group has a plan, the buffer is the plans'
// and the groups' as they are, and the ids have been checked beside this combine
int crec_begin(pg_job* job, char* err, size_t errlen) {
    int rc = combine_begin(job, err, errlen);
    if (rc != PG_OK) return rc;
    const CombineState& c = job->combine;
    if (c.combined_run != job->run_serial) { set_err(err, errlen, "pg_job_combine has not been called for this run"); return PG_ERR_INVALID; }
    bool any = false;
    for (uint32_t g = 0; g + 1 < c.group_off.size(); ++g) any = any || plan_of_group(job, g) != nullptr;
    if (!any) { set_err(err, errlen, "no group's first chain has a record plan on its index contig (pg_job_record_plan)"); return PG_ERR_INVALID; }
    CombinedRecordsState& k = job->crec;
    if (k.dirty) {
        rc = crec_rebuild(job, err, errlen);
        if (rc != PG_OK) return rc;
    }
    if (k.ids_serial != job->combine_serial) rc = crec_check_ids(job, err, errlen);
    return rc;
}

// the records (gl == false) or the GL values of this run's combine are there to be fetched
int crec_ready(pg_job* job, bool gl, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    const CombineState& c = job->combine;
    const CombinedRecordsState& k = job->crec;
    if (!c.planned || c.combined_run != job->run_serial || !k.d || k.dirty || (gl ? k.gl_serial : k.calls_serial) != job->combine_serial) {
        set_err(err, errlen, "%s has not been called for this run's pg_job_combine", gl ? "pg_job_combined_record_gl" : "pg_job_combined_record_calls");
        return PG_ERR_INVALID;
    }
    return PG_OK;
}

// where group g's elements lie, and how many
const unsigned char* crec_slice(const CombinedRecordsState& k, bool gl, uint32_t g, uint64_t* n) {
    const std::vector<uint64_t>& first = gl ? k.gl_first : k.rec_first;
    *n = first[g + 1] - first[g];
    return k.d + (gl ? k.o_gl : 0) + first[g] * (gl ? sizeof(pg_gl) : sizeof(pg_call));
}

int crec_fetch_group(pg_job* job, bool gl, uint32_t g, void* out, char* err, size_t errlen) {
    int rc = crec_ready(job, gl, err, errlen);
    if (rc != PG_OK) return rc;
    const CombinedRecordsState& k = job->crec;
    if (g + 1 >= k.rec_first.size()) { set_err(err, errlen, "group %u of %zu", g, k.rec_first.size() - 1); return PG_ERR_INVALID; }
    uint64_t n = 0;
    const unsigned char* src = crec_slice(k, gl, g, &n);
    if (n == 0) return PG_OK;
    if (!out) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    HIP_TRY(hipMemcpy(out, src, n * (gl ? sizeof(pg_gl) : sizeof(pg_call)), hipMemcpyDeviceToHost));
    return PG_OK;
}

int crec_fetch_groups(pg_job* job, bool gl, void* const* outs, char* err, size_t errlen) {
    int rc = crec_ready(job, gl, err, errlen);
    if (rc != PG_OK) return rc;
    if (!outs) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const CombinedRecordsState& k = job->crec;
    HIP_TRY(hipSetDevice(job->device));
    for (uint32_t g = 0; g + 1 < k.rec_first.size(); ++g) {
        uint64_t n = 0;
        const unsigned char* src = crec_slice(k, gl, g, &n);
        if (n == 0) continue;
        if (!outs[g]) { set_err(err, errlen, "no buffer for group %u", g); return PG_ERR_INVALID; }
        HIP_TRY(hipMemcpyAsync(outs[g], src, n * (gl ? sizeof(pg_gl) : sizeof(pg_call)), hipMemcpyDeviceToHost, job->stream));
    }
    HIP_TRY(hipStreamSynchronize(job->stream));
    return PG_OK;
}

int crec_device_group(pg_job* job, bool gl, uint32_t g, void** d_out, uint64_t* n) {
    if (crec_ready(job, gl, nullptr, 0) != PG_OK || g + 1 >= job->crec.rec_first.size()) return PG_ERR_INVALID;
    uint64_t count = 0;
    const unsigned char* src = crec_slice(job->crec, gl, g, &count);
    if (d_out) *d_out = (void*)src;
    if (n) *n = count;
    return PG_OK;
}

}  // namespace

extern "C" int pg_job_combined_record_calls(pg_job* job, char* err, size_t errlen) {
    int rc = crec_begin(job, err, errlen);
    if (rc != PG_OK) return rc;
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    rc = gq_table_on(job->device, &d_tm, &d_te, err, errlen);
    if (rc != PG_OK) return rc;
    CombinedRecordsState& k = job->crec;
    rc = timed(job, [&](hipStream_t s) {
        pgk_launch_crcalls(job->d_contigs, (const CRecDesc*)(k.d + k.o_desc), (uint32_t)k.desc.size(), k.blocks, k.d + k.o_wide, k.wide, k.d + k.o_stage,
                           k.max_bins, k.stride, k.slots, d_tm, d_te, s);
    }, &k.calls_ms, err, errlen);
    if (rc == PG_OK) k.calls_serial = job->combine_serial;
    return rc;
}

extern "C" int pg_job_combined_record_gl(pg_job* job, char* err, size_t errlen) {
    int rc = crec_begin(job, err, errlen);
    if (rc != PG_OK) return rc;
    CombinedRecordsState& k = job->crec;
    rc = timed(job, [&](hipStream_t s) {
        pgk_launch_crgl(job->d_contigs, (const CRecDesc*)(k.d + k.o_desc), (uint32_t)k.desc.size(), k.blocks, k.d + k.o_wide, k.wide, k.d + k.o_stage,
                        k.max_bins, k.stride, k.slots, s);
    }, &k.gl_ms, err, errlen);
    if (rc == PG_OK) k.gl_serial = job->combine_serial;
    return rc;
}

extern "C" int pg_job_fetch_combined_record_calls(pg_job* job, uint32_t group, pg_call* out, char* err, size_t errlen) { return crec_fetch_group(job, false, group, out, err, errlen); }
extern "C" int pg_job_fetch_combined_record_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen) { return crec_fetch_groups(job, false, (void* const*)outs, err, errlen); }
extern "C" int pg_job_device_combined_record_calls(pg_job* job, uint32_t group, void** d_calls, uint64_t* n) { return crec_device_group(job, false, group, d_calls, n); }
extern "C" int pg_job_fetch_combined_record_gl(pg_job* job, uint32_t group, pg_gl* out, char* err, size_t errlen) { return crec_fetch_group(job, true, group, out, err, errlen); }
extern "C" int pg_job_fetch_combined_record_gl_all(pg_job* job, pg_gl* const* outs, char* err, size_t errlen) { return crec_fetch_groups(job, true, (void* const*)outs, err, errlen); }
extern "C" int pg_job_device_combined_record_gl(pg_job* job, uint32_t group, void** d_gl, uint64_t* n) { return crec_device_group(job, true, group, d_gl, n); }
extern "C" double pg_job_combined_record_calls_ms(const pg_job* job) { return job ? job->crec.calls_ms : 0.0; }
extern "C" double pg_job_combined_record_gl_ms(const pg_job* job) { return job ? job->crec.gl_ms : 0.0; }

// The unit entry points: one contig's combined bins and a plan in, through the same kernels.
namespace {

int records_from_combined(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id, const pg_combined_bin* bins,
                          const pg_record_plan* plan, void* out, bool gl) {
    std::vector<uint64_t> goff(1, 0);
    if (n_variants) {
        if (!allele_id || !bins) return PG_ERR_INVALID;
        const int rc = layout_check(n_variants, allele_off, &goff);
        if (rc != PG_OK) return rc;
    }
    RecordPlanHost h;
    int rc = check_record_plan(plan, n_variants, &h, nullptr, 0);
    if (rc == PG_OK && n_variants) rc = check_record_plan_ids(h, allele_off, allele_id, nullptr, 0);
    if (rc != PG_OK || n_variants == 0) return rc;
    const size_t V1 = (size_t)n_variants + 1, sumA = allele_off[n_variants], n_lik = goff[n_variants];
    if (!combined_bins_ok(bins, n_lik) || !out) return PG_ERR_INVALID;
    rc = select_device(device);
    if (rc != PG_OK) return rc;
    const uint64_t* d_tm = nullptr;
    const int32_t* d_te = nullptr;
    if (!gl) {
        rc = gq_table_on(device, &d_tm, &d_te, nullptr, 0);
        if (rc != PG_OK) return rc;
    }
    RcallsLaunch L;
    plan_rcalls(1, [&](uint32_t) -> const RecordPlanHost* { return &h; }, [&](uint32_t) { return allele_off; }, pgk_combined_records_block(), &L);
    const std::vector<uint64_t> gl_off = record_gl_offsets(h);
    DevContig dc;
    memset(&dc, 0, sizeof(dc));
    CRecDesc cd;
    memset(&cd, 0, sizeof(cd));
    Staged st;
    const size_t p_dc = st.add(sizeof(dc), &dc), p_desc = st.add(sizeof(cd), &cd), p_wide = st.add(L.wide.size() * 4, L.wide.data()),
                 p_aoff = st.add(V1 * 4, allele_off), p_aid = st.add(sumA * 2, allele_id), p_goff = st.add(V1 * 8, goff.data()),
                 p_bins = st.add(n_lik * sizeof(pg_combined_bin), bins), p_plan = st.add(record_plan_device_bytes(h)),
                 p_stage = st.add((size_t)L.n_slots * L.stride * 16), p_gloff = st.add(gl_off.size() * 8, gl_off.data()),
                 p_out = st.add(gl ? (size_t)gl_off.back() * sizeof(pg_gl) : (size_t)h.R * sizeof(pg_call));
    rc = st.alloc();
    if (rc != PG_OK) return rc;
    dc.V = n_variants;
    dc.allele_off = (const uint32_t*)st.at(p_aoff);
    dc.allele_id = (const uint16_t*)st.at(p_aid);
    dc.geno_off = (const uint64_t*)st.at(p_goff);
    cd.blk0 = 0; cd.R = h.R;
    cd.bins = st.at(p_bins);
    cd.calls = st.at(p_out);
    cd.gl = st.at(p_out);
    cd.gl_off = (const uint64_t*)st.at(p_gloff);
    if (!record_plan_upload(h, st.at(p_plan), &cd.plan)) return PG_ERR_DEVICE;
    rc = st.copy_in();
    if (rc != PG_OK) return rc;
    if (gl)
        pgk_launch_crgl((const DevContig*)st.at(p_dc), (const CRecDesc*)st.at(p_desc), 1, L.n_blocks, st.at(p_wide), (uint32_t)(L.wide.size() / 2), st.at(p_stage),
                        L.max_bins, L.stride, L.n_slots, nullptr);
    else
        pgk_launch_crcalls((const DevContig*)st.at(p_dc), (const CRecDesc*)st.at(p_desc), 1, L.n_blocks, st.at(p_wide), (uint32_t)(L.wide.size() / 2), st.at(p_stage),
                           L.max_bins, L.stride, L.n_slots, d_tm, d_te, nullptr);
    return st.read_back(out, p_out);
}

}  // namespace

extern "C" int pg_record_calls_from_combined(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id, const pg_combined_bin* bins,
                                             const pg_record_plan* plan, pg_call* out) {
    return records_from_combined(device, n_variants, allele_off, allele_id, bins, plan, out, false);
}

extern "C" int pg_record_gl_from_combined(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id, const pg_combined_bin* bins,
                                          const pg_record_plan* plan, pg_gl* out) {
    return records_from_combined(device, n_variants, allele_off, allele_id, bins, plan, out, true);
}
