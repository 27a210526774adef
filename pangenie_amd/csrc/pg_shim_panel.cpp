// pg_shim_panel.cpp — the C-ABI of the sample columns of the sampled-panel VCF (pg_panel_text.hip): the bytes
// of every record's cells formed from the reduced panel a chain holds on the device (pg_job_panel_text) and the unit entry
// point over host arrays.  The fetches of the text are those of the record text (pg_shim_calls.cpp: text_family_*), the
// lines over it those of pg_shim_lines.cpp.  Host code off the critical path.
#include <hip/hip_runtime_api.h>

#include <string.h>

#include <vector>

#include "../../include/pangenie_hmm.h"
#include "pg_device.h"
#include "pg_job.h"
#include "pg_launch.h"
#include "pg_panel.h"

using namespace pgj;

namespace {

// Where the arrays of one launch lie in ONE buffer: the packed text (`cap` bytes), then the offsets, the records' UK, the
// scan's arrays, the descriptors, the word of the map check (and, a job's first forming: the id check's descriptors and word).
struct PanelLayout {
    size_t o_off, o_uk, o_bsum, o_bbase, o_desc, o_bad, total;
    PanelLayout(uint64_t cap, uint64_t R, uint32_t n_blocks, size_t n_desc) {
        o_off = align_up((size_t)cap + 16);
        o_uk = o_off + align_up(((size_t)R + 1) * 8 + 8);
        o_bsum = o_uk + align_up((size_t)R * 2 + 8);
        o_bbase = o_bsum + align_up((size_t)n_blocks * 4 + 8);
        o_desc = o_bbase + align_up(((size_t)n_blocks + 1) * 8 + 8);
        o_bad = o_desc + align_up(n_desc * sizeof(PanelDesc) + 8);
        total = o_bad + align_up(8);
    }
};

void panel_launch(unsigned char* d, const PanelLayout& L, uint32_t n_desc, uint32_t n_blocks, uint64_t R, uint64_t cap, hipStream_t s) {
    pgk_launch_ptpanel((const PanelDesc*)(d + L.o_desc), n_desc, n_blocks, (uint32_t*)(d + L.o_bsum), (uint64_t*)(d + L.o_bbase), (uint64_t*)(d + L.o_off), R, (char*)d,
                       cap, (uint32_t*)(d + L.o_bad), s);
}

// blocks of `cells` cells; false if they do not fit 32 bits behind `blk`
bool add_blocks(uint64_t cells, uint32_t* blk) {
    const uint64_t per = pgk_ptpanel_block(), n = (cells + per - 1) / per;
    if (n + *blk >= 0x80000000ull) return false;
    *blk += (uint32_t)n;
    return true;
}

}  // namespace

extern "C" uint64_t pg_panel_text_bound(uint64_t n_records, uint64_t n_paths) { return pgx_panel_text_bound(n_records, n_paths); }

extern "C" int pg_job_panel_text(pg_job* job, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    const uint32_t n = (uint32_t)job->chains.size();
    for (uint32_t c = 0; c < n; ++c) {   // (before anything touches the device: the drivers then take the host route)
        const RecordPlanHost* h = plan_of_chain(job, c);
        const uint32_t P = job->index[job->chains[c].index].H;
        if (h && h->R && P > PGX_PANEL_MAX_PATHS) { set_err(err, errlen, "chain %u has %u paths: the panel text is formed for at most %u", c, P, PGX_PANEL_MAX_PATHS); return PG_ERR_UNSUPPORTED; }
    }
    HIP_TRY(hipSetDevice(job->device));
    if (!job->calls_events) {
        HIP_TRY(hipEventCreate(&job->ev_calls[0]));
        HIP_TRY(hipEventCreate(&job->ev_calls[1]));
        job->calls_events = true;
    }
    RecordTextFamily& f = job->paneltext;
    if (f.dirty) {   // a plan, the index or the panel has changed: the descriptors are made anew, the ids checked on the device
        std::vector<uint64_t> first((size_t)n + 1, 0);
        std::vector<PanelDesc> desc;
        uint32_t blk = 0;
        uint64_t cap = 0;
        for (uint32_t c = 0; c < n; ++c) {
            const RecordPlanHost* h = plan_of_chain(job, c);
            const IndexHost& x = job->index[job->chains[c].index];
            const uint32_t R = h && x.H ? h->R : 0;
            first[c + 1] = first[c] + R;
            if (R == 0) continue;   // (a chain whose index contig has no plan is left out)
            PanelDesc d;
            memset(&d, 0, sizeof(d));
            d.blk0 = blk; d.R = R; d.rec0 = first[c]; d.chain = c; d.P = x.H;
            d.path_allele = (const uint16_t*)(job->arena + x.o_pa);
            d.kmer_off = (const uint32_t*)(job->arena + x.o_koff);
            d.plan = h->dev;
            desc.push_back(d);
            if (!add_blocks((uint64_t)R * x.H, &blk)) { set_err(err, errlen, "the job's panels hold more cells than one launch takes"); return PG_ERR_UNSUPPORTED; }
            cap += pgx_panel_text_bound(R, x.H);
        }
        const uint64_t R = first[n];
        const PanelLayout L(cap, R, blk, desc.size());
        // the id check reads the descriptors of the record calls: a copy of them and its word behind the text's own arrays
        RcallsLaunch ids;
        if (!job->rplan_ids_ok)
            plan_rcalls(n, [&](uint32_t c) { return plan_of_chain(job, c); }, [&](uint32_t c) { return job->index[job->chains[c].index].aoff.data(); }, pgk_calls_block(), &ids);
        const size_t o_ids = L.total, o_hit = o_ids + align_up(ids.desc.size() * sizeof(RCallsDesc) + 8), total = o_hit + align_up(8);
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the panel text failed", total); return PG_ERR_NOMEM; }
        for (PanelDesc& pd : desc) pd.uk = (uint16_t*)(d + L.o_uk) + pd.rec0;
        hipError_t he = hipSuccess;
        if (!desc.empty()) he = hipMemcpy(d + L.o_desc, desc.data(), desc.size() * sizeof(PanelDesc), hipMemcpyHostToDevice);
        if (he == hipSuccess && !ids.desc.empty()) he = hipMemcpy(d + o_ids, ids.desc.data(), ids.desc.size() * sizeof(RCallsDesc), hipMemcpyHostToDevice);
        if (he != hipSuccess) { hipFree(d); set_err(err, errlen, "upload of the panel text's descriptors failed: %s", hipGetErrorString(he)); return PG_ERR_DEVICE; }
        const int rc = check_record_plan_ids_on_device(job, (const RCallsDesc*)(d + o_ids), (uint32_t)ids.desc.size(), ids.n_blocks, d + o_hit, err, errlen);
        if (rc != PG_OK) { hipFree(d); return rc; }
        f.OutputFamily::release();
        f.d = d;
        f.first = std::move(first);
        f.blocks = blk;
        f.o_off = L.o_off; f.o_uk = L.o_uk; f.o_bsum = L.o_bsum; f.o_bbase = L.o_bbase; f.o_desc = L.o_desc;
        f.n_records = R; f.cap = cap;
        f.dirty = false;
        job->panel_desc = std::move(desc);
    }
    const std::vector<PanelDesc>& desc = job->panel_desc;
    const PanelLayout L(f.cap, f.n_records, f.blocks, desc.size());
    f.formed = false;
    hipStream_t s = job->stream;
    HIP_TRY(hipMemsetAsync(f.d + L.o_bad, 0, 8, s));
    HIP_TRY(hipEventRecord(job->ev_calls[0], s));
    panel_launch(f.d, L, (uint32_t)desc.size(), f.blocks, f.n_records, f.cap, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev_calls[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, job->ev_calls[0], job->ev_calls[1]));
    f.ms = ms;
    f.text_first.assign((size_t)n + 1, 0);
    if (!desc.empty() && f.blocks) {
        uint32_t bad = 0;
        HIP_TRY(hipMemcpy(&bad, f.d + L.o_bad, 4, hipMemcpyDeviceToHost));
        if (bad) { set_err(err, errlen, "a path of the panel carries an allele id outside the map of one of its bubble's records"); return PG_ERR_INVALID; }
        std::vector<uint64_t> bbase((size_t)f.blocks + 1);
        HIP_TRY(hipMemcpy(bbase.data(), f.d + L.o_bbase, bbase.size() * 8, hipMemcpyDeviceToHost));
        if (bbase.back() > f.cap) { set_err(err, errlen, "the panel text takes %llu bytes, more than its bound %llu", (unsigned long long)bbase.back(), (unsigned long long)f.cap); return PG_ERR_DEVICE; }
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

extern "C" double pg_job_panel_text_ms(const pg_job* job) { return job ? job->paneltext.ms : 0.0; }

extern "C" int pg_job_panel_text_first(pg_job* job, uint64_t* record_first, uint64_t* text_first, char* err, size_t errlen) {
    int rc = text_family_ready(job, kPanelText, err, errlen);
    if (rc != PG_OK) return rc;
    if (!record_first && !text_first) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const RecordTextFamily& f = job->paneltext;
    if (record_first) memcpy(record_first, f.first.data(), f.first.size() * sizeof(uint64_t));
    if (text_first) memcpy(text_first, f.text_first.data(), f.text_first.size() * sizeof(uint64_t));
    return PG_OK;
}
extern "C" int pg_job_fetch_panel_text(pg_job* job, uint32_t ci, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return text_family_fetch_chain(job, kPanelText, ci, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_fetch_panel_text_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return text_family_fetch_packed(job, kPanelText, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_device_panel_text(pg_job* job, uint32_t ci, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes) {
    return text_family_device(job, kPanelText, ci, d_off, d_text, n_records, n_bytes);
}

// every record's UK (the panel's own count of its bubble), all chains from one copy: what the INFO column of a line needs
extern "C" int pg_job_fetch_panel_uk_packed(pg_job* job, uint16_t* uk, uint64_t n_records, char* err, size_t errlen) {
    int rc = text_family_ready(job, kPanelText, err, errlen);
    if (rc != PG_OK) return rc;
    const RecordTextFamily& f = job->paneltext;
    if (n_records != f.n_records) { set_err(err, errlen, "the text holds %llu records, not %llu", (unsigned long long)f.n_records, (unsigned long long)n_records); return PG_ERR_INVALID; }
    if (n_records == 0) return PG_OK;
    if (!uk) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    HIP_TRY(hipMemcpy(uk, f.d + f.o_uk, (size_t)n_records * 2, hipMemcpyDeviceToHost));
    return PG_OK;
}

// The unit entry point: a plan and a panel's path alleles in, the packed text and its offsets out, through the same kernels.
extern "C" int pg_panel_text_from_paths(int device, const pg_record_plan* plan, uint32_t n_paths, const uint16_t* path_allele, uint64_t* off, char* text,
                                        uint64_t cap) {
    RecordPlanHost h;
    int rc = check_record_plan(plan, plan ? plan->n_variants : 0, &h, nullptr, 0);   // (a malformed plan, 2^31 records or more)
    if (rc != PG_OK) return rc;
    if (!off || n_paths == 0) return PG_ERR_INVALID;
    if (n_paths > PGX_PANEL_MAX_PATHS) return PG_ERR_UNSUPPORTED;
    if (h.V && !path_allele) return PG_ERR_INVALID;
    const uint64_t bound = pgx_panel_text_bound(h.R, n_paths);
    if (cap < bound || (bound && !text)) return PG_ERR_INVALID;
    for (uint32_t v = 0; v < h.V; ++v)   // a path's allele id has an entry in the map of each of its bubble's records
        for (uint32_t q = h.rec_off[v]; q < h.rec_off[v + 1]; ++q) {
            const uint32_t len = h.map_off[q + 1] - h.map_off[q];
            for (uint32_t p = 0; p < n_paths; ++p)
                if (path_allele[(size_t)v * n_paths + p] >= len) return PG_ERR_INVALID;
        }
    if (h.R == 0) { off[0] = 0; return PG_OK; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return PG_ERR_DEVICE; }
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return PG_ERR_DEVICE;
    uint32_t n_blocks = 0;
    if (!add_blocks((uint64_t)h.R * n_paths, &n_blocks)) return PG_ERR_UNSUPPORTED;
    const PanelLayout L(bound, h.R, n_blocks, 1);
    // the inputs behind the launch's own arrays
    const size_t pa_bytes = (size_t)h.V * n_paths * 2;
    const size_t o_plan = L.total, o_pa = o_plan + align_up(record_plan_device_bytes(h) + 8), total = o_pa + align_up(pa_bytes + 8);
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); return PG_ERR_NOMEM; }
    PanelDesc desc;
    memset(&desc, 0, sizeof(desc));
    desc.R = h.R; desc.P = n_paths;
    desc.path_allele = (const uint16_t*)(d + o_pa);
    bool ok = record_plan_upload(h, d + o_plan, &desc.plan) && hipMemcpy(d + L.o_desc, &desc, sizeof(desc), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_pa, path_allele, pa_bytes, hipMemcpyHostToDevice) == hipSuccess && hipMemset(d + L.o_bad, 0, 8) == hipSuccess;
    uint32_t bad = 0;
    if (ok) {
        panel_launch(d, L, 1, n_blocks, h.R, bound, nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
             hipMemcpy(&bad, d + L.o_bad, 4, hipMemcpyDeviceToHost) == hipSuccess && bad == 0 &&
             hipMemcpy(off, d + L.o_off, ((size_t)h.R + 1) * 8, hipMemcpyDeviceToHost) == hipSuccess && off[h.R] <= bound &&
             (off[h.R] == 0 || hipMemcpy(text, d, off[h.R], hipMemcpyDeviceToHost) == hipSuccess);
    }
    hipFree(d);
    return ok ? PG_OK : PG_ERR_DEVICE;
}
