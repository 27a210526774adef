// pg_shim_phase.cpp — the C-ABI of the phasing column of a run_phasing job (pg_phase_text.hip): two numbers
// per VCF record from the Viterbi haplotypes the run left on the device (pg_job_record_phase), the bytes of `GT:KC` formed
// from them (pg_job_phased_text), and the unit entry points over host arrays.  The fetches of the text are those of the
// record text (pg_shim_calls.cpp: text_family_*), the lines over it those of pg_shim_lines.cpp.  Host code off the critical path.
#include <hip/hip_runtime_api.h>

#include <string.h>

#include <vector>

#include "../../include/pangenie_hmm.h"
#include "pg_device.h"
#include "pg_job.h"
#include "pg_launch.h"
#include "pg_phase.h"

using namespace pgj;

static_assert(sizeof(pg_phase) == 4, "pg_phase is the 4-byte record k_rphase stores");

namespace {

// What both formations open with: the job runs the phasing and has run, its device is current, the two events the output
// families share exist.
int phase_begin(pg_job* job, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->params.run_phasing) { set_err(err, errlen, "the job does not run the phasing: it has no haplotypes to form the column from"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    if (!job->calls_events) {
        HIP_TRY(hipEventCreate(&job->ev_calls[0]));
        HIP_TRY(hipEventCreate(&job->ev_calls[1]));
        job->calls_events = true;
    }
    return PG_OK;
}

// launch(stream) between the two events on the job's stream, waited for; its time goes to the family
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
    return PG_OK;
}

bool phase_current(const pg_job* job) {
    const OutputFamily& f = job->rphase;
    return job->ran && f.formed && !f.dirty && f.run == job->run_serial;
}

int phase_ready(pg_job* job, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!job->ran) { set_err(err, errlen, "pg_job_run has not been called"); return PG_ERR_INVALID; }
    if (!phase_current(job)) { set_err(err, errlen, "pg_job_record_phase has not been called for this run and these plans"); return PG_ERR_INVALID; }
    return PG_OK;
}

// Where the arrays of one launch of the text lie in ONE buffer: the packed text (`cap` bytes), then the offsets, the scan's
// arrays and the descriptors.
struct PTextLayout {
    size_t o_off, o_loc, o_bsum, o_bbase, o_desc, total;
    PTextLayout(uint64_t cap, uint64_t R, uint32_t n_blocks, size_t n_desc) {
        o_off = align_up((size_t)cap + 16);
        o_loc = o_off + align_up(((size_t)R + 1) * 8 + 8);
        o_bsum = o_loc + align_up((size_t)R * 4 + 8);
        o_bbase = o_bsum + align_up((size_t)n_blocks * 4 + 8);
        o_desc = o_bbase + align_up(((size_t)n_blocks + 1) * 8 + 8);
        total = o_desc + align_up(n_desc * sizeof(PTextDesc) + 8);
    }
};

void ptext_launch(const DevContig* d_contigs, unsigned char* d, const PTextLayout& L, uint32_t n_desc, uint32_t n_blocks, uint64_t R, uint64_t cap, hipStream_t s) {
    pgk_launch_ptext(d_contigs, (const PTextDesc*)(d + L.o_desc), n_desc, n_blocks, (uint32_t*)(d + L.o_loc), (uint32_t*)(d + L.o_bsum), (uint64_t*)(d + L.o_bbase),
                     (uint64_t*)(d + L.o_off), R, (char*)d, cap, s);
}

bool device_there(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return false; }
    return device >= 0 && device < ndev && hipSetDevice(device) == hipSuccess;
}

}  // namespace

extern "C" uint64_t pg_phase_text_bound(uint64_t n_records) { return pgx_phase_text_bound(n_records); }

// ---------------------------------------------------------------------------------------
//  The record phase: pg_phase per VCF record (k_rphase).
// ---------------------------------------------------------------------------------------
extern "C" int pg_job_record_phase(pg_job* job, char* err, size_t errlen) {
    int rc = phase_begin(job, err, errlen);
    if (rc != PG_OK) return rc;
    OutputFamily& f = job->rphase;
    const uint32_t n = (uint32_t)job->chains.size();
    if (f.dirty) {   // a plan or the index has changed: the descriptors are made anew, the ids checked on the device
        const uint32_t per = pgk_ptext_block();
        std::vector<uint64_t> first((size_t)n + 1, 0);
        std::vector<RPhaseDesc> desc;
        uint32_t blk = 0;
        for (uint32_t c = 0; c < n; ++c) {
            const RecordPlanHost* h = plan_of_chain(job, c);
            const uint32_t R = h ? h->R : 0;
            first[c + 1] = first[c] + R;
            if (R == 0) continue;   // (a chain whose index contig has no plan is left out)
            RPhaseDesc d;
            memset(&d, 0, sizeof(d));
            d.blk0 = blk; d.R = R; d.chain = c; d.run_genotyping = job->params.run_genotyping ? 1u : 0u;
            d.plan = h->dev;
            desc.push_back(d);
            blk += (R + per - 1) / per;
        }
        // the id check reads the descriptors of the record calls: a copy of them and its word behind the phase's own (no room
        // for the copy once the ids have passed)
        RcallsLaunch ids;
        if (!job->rplan_ids_ok)
            plan_rcalls(n, [&](uint32_t c) { return plan_of_chain(job, c); }, [&](uint32_t c) { return job->index[job->chains[c].index].aoff.data(); }, pgk_calls_block(), &ids);
        const size_t o_desc = align_up((size_t)first[n] * sizeof(pg_phase) + 8);
        const size_t o_ids = o_desc + align_up(desc.size() * sizeof(RPhaseDesc) + 8);
        const size_t o_hit = o_ids + align_up(ids.desc.size() * sizeof(RCallsDesc) + 8);
        const size_t total = o_hit + align_up(8);
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the record phase failed", total); return PG_ERR_NOMEM; }
        for (RPhaseDesc& pd : desc) pd.out = d + first[pd.chain] * sizeof(pg_phase);
        hipError_t he = hipSuccess;
        if (!desc.empty()) he = hipMemcpy(d + o_desc, desc.data(), desc.size() * sizeof(RPhaseDesc), hipMemcpyHostToDevice);
        if (he == hipSuccess && !ids.desc.empty()) he = hipMemcpy(d + o_ids, ids.desc.data(), ids.desc.size() * sizeof(RCallsDesc), hipMemcpyHostToDevice);
        if (he != hipSuccess) { hipFree(d); set_err(err, errlen, "upload of the record phase's descriptors failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
        rc = check_record_plan_ids_on_device(job, (const RCallsDesc*)(d + o_ids), (uint32_t)ids.desc.size(), ids.n_blocks, d + o_hit, err, errlen);
        if (rc != PG_OK) { hipFree(d); return rc; }
        f.release();
        f.d = d;
        f.first = std::move(first);
        f.blocks = blk;
        f.o_desc = o_desc;
        f.dirty = false;
        job->rphase_desc = std::move(desc);
    }
    f.formed = false;
    rc = timed_launch(job, f, [&](hipStream_t s) {
        pgk_launch_rphase(job->d_contigs, (const RPhaseDesc*)(f.d + f.o_desc), (uint32_t)job->rphase_desc.size(), f.blocks, s);
    }, err, errlen);
    if (rc != PG_OK) return rc;
    f.formed = true;
    f.run = job->run_serial;
    return PG_OK;
}

extern "C" double pg_job_record_phase_ms(const pg_job* job) { return job ? job->rphase.ms : 0.0; }

extern "C" int pg_job_fetch_record_phase(pg_job* job, uint32_t ci, pg_phase* out, char* err, size_t errlen) {
    int rc = phase_ready(job, err, errlen);
    if (rc != PG_OK) return rc;
    if (ci >= job->chains.size()) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const OutputFamily& f = job->rphase;
    const uint64_t n = f.first[ci + 1] - f.first[ci];
    if (n == 0) return PG_OK;   // (nothing to fetch: a null `out` will do)
    if (!out) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    HIP_TRY(hipMemcpy(out, f.d + f.first[ci] * sizeof(pg_phase), n * sizeof(pg_phase), hipMemcpyDeviceToHost));
    return PG_OK;
}

extern "C" int pg_job_fetch_record_phase_all(pg_job* job, pg_phase* const* outs, char* err, size_t errlen) {
    int rc = phase_ready(job, err, errlen);
    if (rc != PG_OK) return rc;
    if (!outs) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    const OutputFamily& f = job->rphase;
    for (size_t ci = 0; ci < job->chains.size(); ++ci) {
        const uint64_t n = f.first[ci + 1] - f.first[ci];
        if (n == 0) continue;
        if (!outs[ci]) { set_err(err, errlen, "no buffer for chain %zu", ci); return PG_ERR_INVALID; }
        HIP_TRY(hipMemcpyAsync(outs[ci], f.d + f.first[ci] * sizeof(pg_phase), n * sizeof(pg_phase), hipMemcpyDeviceToHost, job->stream));
    }
    HIP_TRY(hipStreamSynchronize(job->stream));
    return PG_OK;
}

extern "C" int pg_job_device_record_phase(pg_job* job, uint32_t ci, void** d_phase, uint64_t* n) {
    if (phase_ready(job, nullptr, 0) != PG_OK || ci >= job->chains.size()) return PG_ERR_INVALID;
    const OutputFamily& f = job->rphase;
    if (d_phase) *d_phase = f.d + f.first[ci] * sizeof(pg_phase);
    if (n) *n = f.first[ci + 1] - f.first[ci];
    return PG_OK;
}

// The unit entry point: a plan and the haplotypes per variant in, one pg_phase per record out, through the same kernel.
extern "C" int pg_record_phase_from_haplotypes(int device, const pg_record_plan* plan, const uint16_t* hap1, const uint16_t* hap2, const uint8_t* keyed,
                                               pg_phase* out) {
    RecordPlanHost h;
    int rc = check_record_plan(plan, plan ? plan->n_variants : 0, &h, nullptr, 0);
    if (rc != PG_OK || h.V == 0) return rc;
    if (!hap1 || !hap2 || !keyed || !out) return PG_ERR_INVALID;
    for (uint32_t v = 0; v < h.V; ++v)   // a haplotype's allele id has an entry in the map of each of its bubble's records
        for (uint32_t q = h.rec_off[v]; q < h.rec_off[v + 1]; ++q) {
            const uint32_t len = h.map_off[q + 1] - h.map_off[q];
            if (hap1[v] >= len || hap2[v] >= len) return PG_ERR_INVALID;
        }
    if (!device_there(device)) return PG_ERR_DEVICE;
    const uint32_t per = pgk_ptext_block(), n_blocks = (h.R + per - 1) / per;
    const size_t o_plan = align_up(sizeof(RPhaseDesc) + 8), o_h1 = o_plan + align_up(record_plan_device_bytes(h) + 8), o_h2 = o_h1 + align_up((size_t)h.V * 2 + 8),
                 o_keyed = o_h2 + align_up((size_t)h.V * 2 + 8), o_out = o_keyed + align_up((size_t)h.V + 8), total = o_out + align_up((size_t)h.R * sizeof(pg_phase) + 8);
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); return PG_ERR_NOMEM; }
    RPhaseDesc desc;
    memset(&desc, 0, sizeof(desc));
    desc.R = h.R;
    desc.out = d + o_out;
    desc.hap1 = (const uint16_t*)(d + o_h1); desc.hap2 = (const uint16_t*)(d + o_h2); desc.keyed = d + o_keyed;
    bool ok = record_plan_upload(h, d + o_plan, &desc.plan) && hipMemcpy(d, &desc, sizeof(desc), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_h1, hap1, (size_t)h.V * 2, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_h2, hap2, (size_t)h.V * 2, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_keyed, keyed, h.V, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        pgk_launch_rphase(nullptr, (const RPhaseDesc*)d, 1, n_blocks, nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
             hipMemcpy(out, d + o_out, (size_t)h.R * sizeof(pg_phase), hipMemcpyDeviceToHost) == hipSuccess;
    }
    hipFree(d);
    return ok ? PG_OK : PG_ERR_DEVICE;
}

// ---------------------------------------------------------------------------------------
//  The phased text: the bytes of the GT:KC column (k_ptext_len / k_ptext_sums / k_ptext_emit).
// ---------------------------------------------------------------------------------------
extern "C" int pg_job_phased_text(pg_job* job, int ignore_imputed, char* err, size_t errlen) {
    int rc = phase_begin(job, err, errlen);
    if (rc != PG_OK) return rc;
    if (!phase_current(job) && (rc = pg_job_record_phase(job, err, errlen)) != PG_OK) return rc;
    RecordTextFamily& f = job->ptext;
    const uint32_t n = (uint32_t)job->chains.size();
    if (f.dirty) {   // a plan or the index has changed: the phase above has been rebuilt, this family follows it
        std::vector<PTextDesc> desc;
        for (const RPhaseDesc& p : job->rphase_desc) {   // (the same records a block: the blocks are the phase's)
            PTextDesc d;
            memset(&d, 0, sizeof(d));
            d.blk0 = p.blk0; d.R = p.R; d.rec0 = job->rphase.first[p.chain]; d.chain = p.chain;
            d.run_genotyping = p.run_genotyping;
            d.phase = p.out; d.rec_var = p.plan.rec_var;
            desc.push_back(d);
        }
        const uint64_t R = job->rphase.first[n], cap = pgx_phase_text_bound(R);
        const PTextLayout L(cap, R, job->rphase.blocks, desc.size());
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, L.total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the phased text failed", L.total); return PG_ERR_NOMEM; }
        f.OutputFamily::release();
        f.d = d;
        f.first = job->rphase.first;
        f.blocks = job->rphase.blocks;
        f.o_off = L.o_off; f.o_loc = L.o_loc; f.o_bsum = L.o_bsum; f.o_bbase = L.o_bbase; f.o_desc = L.o_desc;
        f.n_records = R; f.cap = cap;
        f.dirty = false;
        job->ptext_desc = std::move(desc);
    }
    std::vector<PTextDesc>& desc = job->ptext_desc;
    for (PTextDesc& d : desc) d.ignore_imputed = ignore_imputed ? 1u : 0u;
    const PTextLayout L(f.cap, f.n_records, f.blocks, desc.size());
    if (!desc.empty()) HIP_TRY(hipMemcpyAsync(f.d + L.o_desc, desc.data(), desc.size() * sizeof(PTextDesc), hipMemcpyHostToDevice, job->stream));
    f.formed = false;
    rc = timed_launch(job, f, [&](hipStream_t s) { ptext_launch(job->d_contigs, f.d, L, (uint32_t)desc.size(), f.blocks, f.n_records, f.cap, s); }, err, errlen);
    if (rc != PG_OK) return rc;
    f.text_first.assign((size_t)n + 1, 0);
    if (!desc.empty() && f.blocks) {
        std::vector<uint64_t> bbase((size_t)f.blocks + 1);
        HIP_TRY(hipMemcpy(bbase.data(), f.d + L.o_bbase, bbase.size() * 8, hipMemcpyDeviceToHost));
        if (bbase.back() > f.cap) { set_err(err, errlen, "the phased text takes %llu bytes, more than its bound %llu", (unsigned long long)bbase.back(), (unsigned long long)f.cap); return PG_ERR_DEVICE; }
        size_t i = 0;   // a chain begins a block: its first byte is that block's
        for (uint32_t c = 0; c < n; ++c) {
            f.text_first[c] = i < desc.size() ? bbase[desc[i].blk0] : bbase.back();
            if (i < desc.size() && desc[i].chain == c) ++i;
        }
        f.text_first[n] = bbase.back();
    }
    f.run = job->run_serial;
    f.formed = true;
    f.serial += 1;
    return PG_OK;
}

extern "C" double pg_job_phased_text_ms(const pg_job* job) { return job ? job->ptext.ms : 0.0; }

extern "C" int pg_job_phased_text_first(pg_job* job, uint64_t* record_first, uint64_t* text_first, char* err, size_t errlen) {
    int rc = text_family_ready(job, kPhasedText, err, errlen);
    if (rc != PG_OK) return rc;
    if (!record_first && !text_first) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const RecordTextFamily& f = job->ptext;
    if (record_first) memcpy(record_first, f.first.data(), f.first.size() * sizeof(uint64_t));
    if (text_first) memcpy(text_first, f.text_first.data(), f.text_first.size() * sizeof(uint64_t));
    return PG_OK;
}
extern "C" int pg_job_fetch_phased_text(pg_job* job, uint32_t ci, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return text_family_fetch_chain(job, kPhasedText, ci, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_fetch_phased_text_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return text_family_fetch_packed(job, kPhasedText, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_device_phased_text(pg_job* job, uint32_t ci, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes) {
    return text_family_device(job, kPhasedText, ci, d_off, d_text, n_records, n_bytes);
}

// The unit entry point: arbitrary fields in, the packed text and its offsets out, through the same kernels.
extern "C" int pg_phase_text_from_fields(int device, uint64_t n_records, const pg_phase* phase, const uint16_t* kc, const uint8_t* no_call, uint64_t* off,
                                         char* text, uint64_t cap) {
    if (!off || n_records >= 0x80000000ull) return PG_ERR_INVALID;
    if (n_records && (!phase || !kc)) return PG_ERR_INVALID;
    if (cap < pgx_phase_text_bound(n_records) || (cap && !text)) return PG_ERR_INVALID;
    for (uint64_t q = 0; q < n_records; ++q)   // what the bound counts on: GT numbers up to 255, or `.`
        if ((phase[q].allele_1 > 255 && phase[q].allele_1 != PG_PHASE_UNDEFINED) || (phase[q].allele_2 > 255 && phase[q].allele_2 != PG_PHASE_UNDEFINED)) return PG_ERR_INVALID;
    if (n_records == 0) { off[0] = 0; return PG_OK; }
    if (!device_there(device)) return PG_ERR_DEVICE;
    const uint32_t per = pgk_ptext_block(), R = (uint32_t)n_records, n_blocks = (R + per - 1) / per;
    const uint64_t bound = pgx_phase_text_bound(n_records);
    const PTextLayout L(bound, R, n_blocks, 1);
    // the inputs behind the launch's own arrays
    const size_t o_phase = L.total, o_kc = o_phase + align_up((size_t)R * 4 + 8), o_nc = o_kc + align_up((size_t)R * 2 + 8), total = o_nc + align_up((size_t)R + 8);
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); return PG_ERR_NOMEM; }
    PTextDesc desc;
    memset(&desc, 0, sizeof(desc));
    desc.R = R;
    desc.phase = d + o_phase; desc.kc = (const uint16_t*)(d + o_kc);
    desc.no_call = no_call ? d + o_nc : nullptr;
    bool ok = hipMemcpy(d + L.o_desc, &desc, sizeof(desc), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_phase, phase, (size_t)R * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_kc, kc, (size_t)R * 2, hipMemcpyHostToDevice) == hipSuccess &&
              (!no_call || hipMemcpy(d + o_nc, no_call, R, hipMemcpyHostToDevice) == hipSuccess);
    if (ok) {
        ptext_launch(nullptr, d, L, 1, n_blocks, R, bound, nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
             hipMemcpy(off, d + L.o_off, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost) == hipSuccess && off[R] <= bound &&
             (off[R] == 0 || hipMemcpy(text, d, off[R], hipMemcpyDeviceToHost) == hipSuccess);
    }
    hipFree(d);
    return ok ? PG_OK : PG_ERR_DEVICE;
}
