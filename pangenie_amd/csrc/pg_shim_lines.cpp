// pg_shim_lines.cpp — the C-ABI of the record lines (pg_record_lines.hip):
// the prefix of an index contig or of a stride of them, plain or slotted, the forming of whole VCF lines from a job's record
// text, their fetches, and the unit entry points over host arrays.  A job has three such families — the lines of the record
// text (GT:GQ:GL:KC), those of the phased text (GT:KC) and those of the panel text (GT, one column per
// selected path), each with prefixes of its own — and ONE
// implementation: every function below the unit entry points' takes the family as a LinesKind row (pg_job.h).  Host code
// off the critical path.
#include <hip/hip_runtime_api.h>

#include <string.h>

#include <vector>

#include "../../include/pangenie_hmm.h"
#include "pg_device.h"
#include "pg_job.h"
#include "pg_launch.h"

using namespace pgj;

namespace {

// Where the arrays of one launch lie in ONE buffer: the packed lines (`cap` bytes), then the offsets, the scan's arrays, the
// descriptors and the members.
struct RLinesLayout {
    size_t o_off, o_loc, o_bsum, o_bbase, o_desc, o_members, total;
    RLinesLayout(uint64_t cap, uint64_t n_lines, uint32_t n_blocks, size_t desc_bytes, size_t n_members) {
        o_off = align_up((size_t)cap + 16);
        o_loc = o_off + align_up(((size_t)n_lines + 1) * 8 + 8);
        o_bsum = o_loc + align_up((size_t)n_lines * 4 + 8);
        o_bbase = o_bsum + align_up((size_t)n_blocks * 4 + 8);
        o_desc = o_bbase + align_up(((size_t)n_blocks + 1) * 8 + 8);
        o_members = o_desc + align_up(desc_bytes + 8);
        total = o_members + align_up(n_members * sizeof(RLinesMember) + 8);
    }
};

// one more contig of R records and S members behind those of `desc`: its blocks of both kernels, its first line and member.
// slotted: the launch's kernels are the slotted ones, whose waves take other runs of lines.
RLinesDesc& rlines_add(std::vector<RLinesDesc>* desc, bool slotted, uint32_t R, uint32_t S, uint32_t* blk, uint32_t* eblk, uint64_t* line, uint32_t* mem) {
    RLinesDesc d;
    memset(&d, 0, sizeof(d));
    const uint32_t per = pgk_rlines_block();
    d.blk0 = *blk; d.R = R; d.eblk0 = *eblk; d.lpw = pgk_rlines_lines_per_wave(S, slotted);
    d.line0 = *line; d.mem0 = *mem; d.S = S;
    *blk += (R + per - 1) / per;
    *eblk += (R + d.lpw - 1) / d.lpw;
    *line += R;
    *mem += S;
    desc->push_back(d);
    return desc->back();
}

void rlines_launch(unsigned char* d, const RLinesLayout& L, bool slotted, const DevContig* d_contigs, uint32_t n_desc, uint32_t n_blocks, uint32_t n_eblocks,
                   uint64_t n_lines, uint64_t cap, hipStream_t s) {
    pgk_launch_rlines(d_contigs, (const RLinesDesc*)(d + L.o_desc), n_desc, (const RLinesMember*)(d + L.o_members), slotted, n_blocks, n_eblocks,
                      (uint32_t*)(d + L.o_loc), (uint32_t*)(d + L.o_bsum), (uint64_t*)(d + L.o_bbase), (uint64_t*)(d + L.o_off), n_lines, (char*)d, cap, s);
}

bool text_current(const pg_job* job, const LinesKind& k) {
    const RecordTextFamily& t = job->*k.text.text;
    return t.formed && !t.dirty && (!k.text.per_run || (job->ran && t.run == job->run_serial));
}

int rlines_ready(pg_job* job, const LinesKind& k, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    const RecordLinesFamily& f = job->*k.lines;
    if (!text_current(job, k) || !f.formed || f.text_serial != (job->*k.text.text).serial) {
        set_err(err, errlen, "%s has not been called for this text and these prefixes", k.former);
        return PG_ERR_INVALID;
    }
    return PG_OK;
}

// lines [l0, l1) of a formed job: their offsets less `minus` and their bytes [b0, b1), n_bytes of them
int rlines_fetch(pg_job* job, const RecordLinesFamily& f, uint64_t l0, uint64_t l1, uint64_t b0, uint64_t b1, uint64_t minus, uint64_t* off, char* text,
                 uint64_t n_bytes, char* err, size_t errlen) {
    if (n_bytes != b1 - b0) { set_err(err, errlen, "the lines hold %llu bytes, not %llu", (unsigned long long)(b1 - b0), (unsigned long long)n_bytes); return PG_ERR_INVALID; }
    if (n_bytes && !text) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    if (off) {
        if (f.n_lines == 0) off[0] = 0;
        else HIP_TRY(hipMemcpyAsync(off, f.d + f.o_off + l0 * 8, (l1 - l0 + 1) * 8, hipMemcpyDeviceToHost, job->stream));
    }
    if (n_bytes) HIP_TRY(hipMemcpyAsync(text, f.d + b0, n_bytes, hipMemcpyDeviceToHost, job->stream));
    HIP_TRY(hipStreamSynchronize(job->stream));
    if (off && minus && f.n_lines)
        for (uint64_t q = 0; q <= l1 - l0; ++q) off[q] -= minus;
    return PG_OK;
}

bool offsets_ok(const uint64_t* off, uint64_t n) {
    if (!off || off[0] != 0) return false;
    for (uint64_t q = 0; q < n; ++q)
        if (off[q + 1] < off[q]) return false;
    return true;
}

}  // namespace

extern "C" uint64_t pg_record_lines_bound(uint64_t n_records, uint64_t n_members, uint64_t prefix_bytes, uint64_t text_bytes) {
    return prefix_bytes + text_bytes + n_records * (n_members + 1);
}
extern "C" uint64_t pg_record_lines_bound_slotted(uint64_t n_records, uint64_t n_members, uint64_t prefix_bytes, uint64_t text_bytes) {
    return pg_record_lines_bound(n_records, n_members, prefix_bytes, text_bytes) + 5 * n_records;   // (UK has 16 bits: at most 5 digits a line)
}

namespace {

// a prefix of R records as the caller handed it in: everything that needs the arrays alone
int check_prefix(uint32_t R, const uint64_t* off, const char* bytes, const uint32_t* slot, char* err, size_t errlen) {
    if (!offsets_ok(off, R)) { set_err(err, errlen, "the prefix offsets are null, do not start at 0 or shrink"); return PG_ERR_INVALID; }
    if (off[R] && !bytes) { set_err(err, errlen, "null prefix bytes"); return PG_ERR_INVALID; }
    if (slot)
        for (uint32_t r = 0; r < R; ++r)
            if (slot[r] > off[r + 1] - off[r]) {
                set_err(err, errlen, "the slot of record %u lies at byte %u of a prefix of %llu bytes", r, slot[r], (unsigned long long)(off[r + 1] - off[r]));
                return PG_ERR_INVALID;
            }
    return PG_OK;
}

// the checked prefix on the job's device, ready to be referred to by index contigs
int prefix_to_device(pg_job* job, const LinesKind& k, uint32_t R, const uint64_t* off, const char* bytes, const uint32_t* slot, LinePrefixRef* ref, char* err,
                     size_t errlen) {
    HIP_TRY(hipSetDevice(job->device));
    LinePrefix p;
    p.R = R; p.bytes = off[R];
    p.o_slot = slot ? align_up(((size_t)R + 1) * 8) : 0;
    p.o_bytes = align_up(((size_t)R + 1) * 8) + (slot ? align_up((size_t)R * 4 + 4) : 0);
    const size_t total = p.o_bytes + (size_t)p.bytes + 16;
    if (hipMalloc((void**)&p.d, total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the line prefix failed", total); return PG_ERR_NOMEM; }
    if (hipMemcpy(p.d, off, ((size_t)R + 1) * 8, hipMemcpyHostToDevice) != hipSuccess ||
        (slot && R && hipMemcpy(p.d + p.o_slot, slot, (size_t)R * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        (p.bytes && hipMemcpy(p.d + p.o_bytes, bytes, p.bytes, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipGetLastError();
        hipFree(p.d);
        set_err(err, errlen, "upload of the line prefix failed");
        return PG_ERR_DEVICE;
    }
    *ref = line_prefix_ref(p);
    RecordLinesFamily& f = job->*k.lines;
    if (f.prefix.size() != job->index.size()) f.prefix.resize(job->index.size());
    if (job->stream) HIP_TRY(hipStreamSynchronize(job->stream));   // (nothing reads the prefixes this one replaces any more)
    return PG_OK;
}

// the prefix of one index contig, plain (slot null) or slotted
int line_prefix(pg_job* job, const LinesKind& k, uint32_t ix, const uint64_t* off, const char* bytes, const uint32_t* slot, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (ix >= job->index.size()) { set_err(err, errlen, "index contig %u of %zu", ix, job->index.size()); return PG_ERR_INVALID; }
    if (ix >= job->rplans.size() || !job->rplans[ix]) { set_err(err, errlen, "index contig %u has no record plan", ix); return PG_ERR_INVALID; }
    const uint32_t R = job->rplans[ix]->R;
    int rc = check_prefix(R, off, bytes, slot, err, errlen);
    if (rc != PG_OK) return rc;
    LinePrefixRef ref;
    rc = prefix_to_device(job, k, R, off, bytes, slot, &ref, err, errlen);
    if (rc != PG_OK) return rc;
    (job->*k.lines).prefix[ix] = std::move(ref);   // (this index contig's reference alone: the members of a stride keep theirs)
    (job->*k.lines).formed = false;
    return PG_OK;
}

}  // namespace

extern "C" int pg_job_line_prefix_slotted(pg_job* job, uint32_t ix, const uint64_t* off, const char* bytes, const uint32_t* slot, char* err, size_t errlen) {
    return line_prefix(job, kRecordLines, ix, off, bytes, slot, err, errlen);
}

extern "C" int pg_job_line_prefix(pg_job* job, uint32_t ix, const uint64_t* off, const char* bytes, char* err, size_t errlen) {
    return line_prefix(job, kRecordLines, ix, off, bytes, nullptr, err, errlen);
}

// (a plain prefix: the slotted kernel prints UK by the genotyping rule, which is not the phasing column's)
extern "C" int pg_job_phased_line_prefix(pg_job* job, uint32_t ix, const uint64_t* off, const char* bytes, char* err, size_t errlen) {
    return line_prefix(job, kPhasedLines, ix, off, bytes, nullptr, err, errlen);
}

namespace {

// one prefix for every member of a stride of index contigs
int line_prefix_strided(pg_job* job, const LinesKind& k, uint32_t contig, uint32_t n_contigs, const uint64_t* off, const char* bytes, const uint32_t* slot,
                        char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (n_contigs == 0 || contig >= n_contigs) { set_err(err, errlen, "contig %u of %u", contig, n_contigs); return PG_ERR_INVALID; }
    if (job->index.size() % n_contigs != 0) { set_err(err, errlen, "the job's %zu index contigs are no multiple of %u contigs", job->index.size(), n_contigs); return PG_ERR_INVALID; }
    if (contig >= job->index.size()) return PG_OK;   // (a job without index contigs: no member)
    for (size_t ix = contig; ix < job->index.size(); ix += n_contigs) {
        if (ix >= job->rplans.size() || !job->rplans[ix]) { set_err(err, errlen, "index contig %zu (member %zu of the stride) has no record plan", ix, ix / n_contigs); return PG_ERR_INVALID; }
        if (job->rplans[ix]->R != job->rplans[contig]->R) {
            set_err(err, errlen, "the plan of index contig %zu (member %zu of the stride) has %u records, that of the first member %u", ix, ix / n_contigs, job->rplans[ix]->R, job->rplans[contig]->R);
            return PG_ERR_INVALID;
        }
    }
    const uint32_t R = job->rplans[contig]->R;
    int rc = check_prefix(R, off, bytes, slot, err, errlen);
    if (rc != PG_OK) return rc;
    LinePrefixRef ref;
    rc = prefix_to_device(job, k, R, off, bytes, slot, &ref, err, errlen);
    if (rc != PG_OK) return rc;
    for (size_t ix = contig; ix < job->index.size(); ix += n_contigs) (job->*k.lines).prefix[ix] = ref;
    (job->*k.lines).formed = false;
    return PG_OK;
}

}  // namespace

extern "C" int pg_job_line_prefix_strided(pg_job* job, uint32_t contig, uint32_t n_contigs, const uint64_t* off, const char* bytes, const uint32_t* slot,
                                          char* err, size_t errlen) {
    return line_prefix_strided(job, kRecordLines, contig, n_contigs, off, bytes, slot, err, errlen);
}

// the prefixes of the panel lines (CHROM .. INFO, GT): a slotted one takes its UK from the panel text's per-record array
extern "C" int pg_job_panel_line_prefix(pg_job* job, uint32_t ix, const uint64_t* off, const char* bytes, char* err, size_t errlen) {
    return line_prefix(job, kPanelLines, ix, off, bytes, nullptr, err, errlen);
}
extern "C" int pg_job_panel_line_prefix_slotted(pg_job* job, uint32_t ix, const uint64_t* off, const char* bytes, const uint32_t* slot, char* err, size_t errlen) {
    return line_prefix(job, kPanelLines, ix, off, bytes, slot, err, errlen);
}
extern "C" int pg_job_panel_line_prefix_strided(pg_job* job, uint32_t contig, uint32_t n_contigs, const uint64_t* off, const char* bytes, const uint32_t* slot,
                                                char* err, size_t errlen) {
    return line_prefix_strided(job, kPanelLines, contig, n_contigs, off, bytes, slot, err, errlen);
}

namespace {

// the lines of every index contig that takes part, joined from the family's text as it is
int form_lines(pg_job* job, const LinesKind& k, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (!text_current(job, k)) { set_err(err, errlen, "%s has not been called for this run and these plans", k.text.former); return PG_ERR_INVALID; }
    HIP_TRY(hipSetDevice(job->device));
    RecordLinesFamily& f = job->*k.lines;
    const RecordTextFamily& t = job->*k.text.text;
    const size_t n_index = job->index.size(), n_chains = job->chains.size();
    f.formed = false;
    // the members of every index contig: its chains in ascending id
    std::vector<std::vector<uint32_t>> chains_of(n_index);
    for (size_t c = 0; c < n_chains; ++c) chains_of[job->chains[c].index].push_back((uint32_t)c);
    auto takes_part = [&](size_t ix) {
        return ix < job->rplans.size() && job->rplans[ix] && ix < f.prefix.size() && f.prefix[ix] && !chains_of[ix].empty() && job->rplans[ix]->R != 0;
    };
    bool slotted = false;   // one slotted prefix among the contigs that take part: the launch is the slotted kernels'
    for (size_t ix = 0; ix < n_index; ++ix) slotted |= takes_part(ix) && f.prefix[ix]->o_slot != 0;
    std::vector<RLinesDesc> desc;
    std::vector<RLinesMember> members;
    std::vector<size_t> contig_of;   // the index contig of every descriptor
    uint32_t blk = 0, eblk = 0, mem = 0;
    uint64_t line = 0, cap = 0;
    for (size_t ix = 0; ix < n_index; ++ix) {
        const bool plan = ix < job->rplans.size() && job->rplans[ix], prefix = ix < f.prefix.size() && f.prefix[ix];
        if (!plan || !prefix || chains_of[ix].empty()) continue;
        const uint32_t R = job->rplans[ix]->R, S = (uint32_t)chains_of[ix].size();
        const LinePrefix& px = *f.prefix[ix];
        if (px.R != R) { set_err(err, errlen, "the prefix of index contig %zu has %u records, its plan %u", ix, px.R, R); return PG_ERR_INVALID; }
        if (R == 0) continue;
        uint64_t text_bytes = 0;
        for (uint32_t c : chains_of[ix]) {
            if (t.first[c + 1] - t.first[c] != R) { set_err(err, errlen, "chain %u holds %llu records of text, its plan %u", c, (unsigned long long)(t.first[c + 1] - t.first[c]), R); return PG_ERR_INVALID; }
            RLinesMember m;
            m.off = (const uint64_t*)(t.d + t.o_off) + t.first[c];   // (absolute in the packed text)
            m.text = (const char*)t.d;
            members.push_back(m);
            text_bytes += t.text_first[c + 1] - t.text_first[c];
        }
        RLinesDesc& d = rlines_add(&desc, slotted, R, S, &blk, &eblk, &line, &mem);
        d.prefix_off = (const uint64_t*)px.d;
        d.prefix = (const char*)(px.d + px.o_bytes);
        if (px.o_slot) {   // UK: the first member's count of the record's bubble
            d.slot = (const uint32_t*)(px.d + px.o_slot);
            if (t.o_uk) d.uk = (const uint16_t*)(t.d + t.o_uk) + t.first[chains_of[ix][0]];   // (the panel text keeps it per record)
            else {
                d.rec_var = job->rplans[ix]->dev.rec_var;
                d.chain = chains_of[ix][0];
            }
        }
        contig_of.push_back(ix);
        cap += px.o_slot ? pg_record_lines_bound_slotted(R, S, px.bytes, text_bytes) : pg_record_lines_bound(R, S, px.bytes, text_bytes);
    }
    const RLinesLayout L(cap, line, blk, desc.size() * sizeof(RLinesDesc), members.size());
    if (!f.d || f.alloc < L.total) {
        unsigned char* d = nullptr;
        if (hipMalloc((void**)&d, L.total) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "hipMalloc of %zu bytes for the record lines failed", L.total); return PG_ERR_NOMEM; }
        f.OutputFamily::release();
        f.d = d;
        f.alloc = L.total;
    }
    f.o_off = L.o_off; f.n_lines = line; f.cap = cap; f.blocks = blk;
    f.line_first.assign(n_index + 1, 0);
    f.byte_first.assign(n_index + 1, 0);
    f.ms = 0.0;
    if (!desc.empty()) {
        hipStream_t s = job->stream;
        HIP_TRY(hipMemcpyAsync(f.d + L.o_desc, desc.data(), desc.size() * sizeof(RLinesDesc), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(f.d + L.o_members, members.data(), members.size() * sizeof(RLinesMember), hipMemcpyHostToDevice, s));
        if (!job->calls_events) {
            HIP_TRY(hipEventCreate(&job->ev_calls[0]));
            HIP_TRY(hipEventCreate(&job->ev_calls[1]));
            job->calls_events = true;
        }
        HIP_TRY(hipEventRecord(job->ev_calls[0], s));
        rlines_launch(f.d, L, slotted, job->d_contigs, (uint32_t)desc.size(), blk, eblk, line, cap, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(job->ev_calls[1], s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, job->ev_calls[0], job->ev_calls[1]));
        f.ms = ms;
        std::vector<uint64_t> bbase((size_t)blk + 1);
        HIP_TRY(hipMemcpy(bbase.data(), f.d + L.o_bbase, bbase.size() * 8, hipMemcpyDeviceToHost));
        if (bbase.back() > cap) { set_err(err, errlen, "the record lines take %llu bytes, more than their bound %llu", (unsigned long long)bbase.back(), (unsigned long long)cap); return PG_ERR_DEVICE; }
        size_t i = 0;   // a contig begins a block: its first byte is that block's
        for (size_t ix = 0; ix < n_index; ++ix) {
            f.line_first[ix] = i < desc.size() ? desc[i].line0 : line;
            f.byte_first[ix] = i < desc.size() ? bbase[desc[i].blk0] : bbase.back();
            if (i < desc.size() && contig_of[i] == ix) ++i;
        }
        f.line_first[n_index] = line;
        f.byte_first[n_index] = bbase.back();
    }
    f.run = job->run_serial;
    f.text_serial = t.serial;
    f.dirty = false;
    f.formed = true;
    return PG_OK;
}

int lines_first(pg_job* job, const LinesKind& k, uint64_t* n_index_contigs, uint64_t* line_first, uint64_t* byte_first, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    if (n_index_contigs) *n_index_contigs = job->index.size();
    if (!line_first && !byte_first) return PG_OK;
    const int rc = rlines_ready(job, k, err, errlen);
    if (rc != PG_OK) return rc;
    const RecordLinesFamily& f = job->*k.lines;
    if (line_first) memcpy(line_first, f.line_first.data(), f.line_first.size() * sizeof(uint64_t));
    if (byte_first) memcpy(byte_first, f.byte_first.data(), f.byte_first.size() * sizeof(uint64_t));
    return PG_OK;
}

int fetch_lines(pg_job* job, const LinesKind& k, uint32_t ix, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    const int rc = rlines_ready(job, k, err, errlen);
    if (rc != PG_OK) return rc;
    if (ix >= job->index.size()) { set_err(err, errlen, "bad argument"); return PG_ERR_INVALID; }
    const RecordLinesFamily& f = job->*k.lines;
    return rlines_fetch(job, f, f.line_first[ix], f.line_first[ix + 1], f.byte_first[ix], f.byte_first[ix + 1], f.byte_first[ix], off, text, n_bytes, err, errlen);
}

int fetch_lines_packed(pg_job* job, const LinesKind& k, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    const int rc = rlines_ready(job, k, err, errlen);
    if (rc != PG_OK) return rc;
    const RecordLinesFamily& f = job->*k.lines;
    return rlines_fetch(job, f, 0, f.n_lines, 0, f.byte_first.back(), 0, off, text, n_bytes, err, errlen);
}

int device_lines(pg_job* job, const LinesKind& k, uint32_t ix, void** d_off, void** d_text, uint64_t* n_lines, uint64_t* n_bytes) {
    if (rlines_ready(job, k, nullptr, 0) != PG_OK || ix >= job->index.size()) return PG_ERR_INVALID;
    const RecordLinesFamily& f = job->*k.lines;
    if (d_off) *d_off = f.d + f.o_off + f.line_first[ix] * 8;
    if (d_text) *d_text = f.d + f.byte_first[ix];
    if (n_lines) *n_lines = f.line_first[ix + 1] - f.line_first[ix];
    if (n_bytes) *n_bytes = f.byte_first[ix + 1] - f.byte_first[ix];
    return PG_OK;
}

}  // namespace

extern "C" int pg_job_record_lines(pg_job* job, char* err, size_t errlen) { return form_lines(job, kRecordLines, err, errlen); }
extern "C" double pg_job_record_lines_ms(const pg_job* job) { return job ? job->rlines.ms : 0.0; }
extern "C" int pg_job_record_lines_first(pg_job* job, uint64_t* n_index_contigs, uint64_t* line_first, uint64_t* byte_first, char* err, size_t errlen) {
    return lines_first(job, kRecordLines, n_index_contigs, line_first, byte_first, err, errlen);
}
extern "C" int pg_job_fetch_record_lines(pg_job* job, uint32_t ix, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return fetch_lines(job, kRecordLines, ix, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_fetch_record_lines_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return fetch_lines_packed(job, kRecordLines, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_device_record_lines(pg_job* job, uint32_t ix, void** d_off, void** d_text, uint64_t* n_lines, uint64_t* n_bytes) {
    return device_lines(job, kRecordLines, ix, d_off, d_text, n_lines, n_bytes);
}

// the lines of the phased text: the same joiner over the family's own prefixes
extern "C" int pg_job_phased_lines(pg_job* job, char* err, size_t errlen) { return form_lines(job, kPhasedLines, err, errlen); }
extern "C" double pg_job_phased_lines_ms(const pg_job* job) { return job ? job->plines.ms : 0.0; }
extern "C" int pg_job_phased_lines_first(pg_job* job, uint64_t* n_index_contigs, uint64_t* line_first, uint64_t* byte_first, char* err, size_t errlen) {
    return lines_first(job, kPhasedLines, n_index_contigs, line_first, byte_first, err, errlen);
}
extern "C" int pg_job_fetch_phased_lines(pg_job* job, uint32_t ix, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return fetch_lines(job, kPhasedLines, ix, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_fetch_phased_lines_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return fetch_lines_packed(job, kPhasedLines, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_device_phased_lines(pg_job* job, uint32_t ix, void** d_off, void** d_text, uint64_t* n_lines, uint64_t* n_bytes) {
    return device_lines(job, kPhasedLines, ix, d_off, d_text, n_lines, n_bytes);
}

// the lines of the panel text: the same joiner over the family's own prefixes
extern "C" int pg_job_panel_lines(pg_job* job, char* err, size_t errlen) { return form_lines(job, kPanelLines, err, errlen); }
extern "C" double pg_job_panel_lines_ms(const pg_job* job) { return job ? job->panellines.ms : 0.0; }
extern "C" int pg_job_panel_lines_first(pg_job* job, uint64_t* n_index_contigs, uint64_t* line_first, uint64_t* byte_first, char* err, size_t errlen) {
    return lines_first(job, kPanelLines, n_index_contigs, line_first, byte_first, err, errlen);
}
extern "C" int pg_job_fetch_panel_lines(pg_job* job, uint32_t ix, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return fetch_lines(job, kPanelLines, ix, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_fetch_panel_lines_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen) {
    return fetch_lines_packed(job, kPanelLines, off, text, n_bytes, err, errlen);
}
extern "C" int pg_job_device_panel_lines(pg_job* job, uint32_t ix, void** d_off, void** d_text, uint64_t* n_lines, uint64_t* n_bytes) {
    return device_lines(job, kPanelLines, ix, d_off, d_text, n_lines, n_bytes);
}

namespace {

// The unit entry points: arbitrary bytes in, the packed lines and their offsets out, through the kernels of a job — the
// slotted ones with `slotted` (slot and uk may then be null: a descriptor without slots), else the plain ones.
int rlines_from_text(int device, uint64_t n_records, uint64_t n_members, const uint64_t* const* off, const char* const* text, const uint64_t* prefix_off,
                     const char* prefix, const uint32_t* slot, const uint16_t* uk, bool slotted, uint64_t* out_off, char* out, uint64_t cap) {
    if (!out_off || !off || !text || !prefix_off || n_members == 0 || n_members >= 0x80000000ull - (slotted ? 4 : 2) || n_records >= 0x80000000ull) return PG_ERR_INVALID;
    if (check_prefix((uint32_t)n_records, prefix_off, prefix, slot, nullptr, 0) != PG_OK || (slot && !uk)) return PG_ERR_INVALID;
    uint64_t text_bytes = 0;
    for (uint64_t s = 0; s < n_members; ++s) {
        if (!offsets_ok(off[s], n_records) || (off[s][n_records] && !text[s])) return PG_ERR_INVALID;
        text_bytes += off[s][n_records];
    }
    const uint64_t bound = slot ? pg_record_lines_bound_slotted(n_records, n_members, prefix_off[n_records], text_bytes)
                                : pg_record_lines_bound(n_records, n_members, prefix_off[n_records], text_bytes);
    if (cap < bound || (cap && !out)) return PG_ERR_INVALID;
    if (n_records == 0) { out_off[0] = 0; return PG_OK; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return PG_ERR_DEVICE; }
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return PG_ERR_DEVICE;
    const uint32_t R = (uint32_t)n_records, S = (uint32_t)n_members;
    std::vector<RLinesDesc> desc;
    uint32_t blk = 0, eblk = 0, mem = 0;
    uint64_t line = 0;
    rlines_add(&desc, slotted, R, S, &blk, &eblk, &line, &mem);
    const RLinesLayout L(bound, R, blk, sizeof(RLinesDesc), S);
    // the inputs behind the launch's own arrays: the prefix (offsets, bytes, slots, UK), then member after member (offsets, bytes)
    const size_t offs_bytes = align_up(((size_t)R + 1) * 8);
    std::vector<size_t> o_moff(S), o_mtext(S);
    size_t at = L.total;
    const size_t o_poff = at; at += offs_bytes;
    const size_t o_pbytes = at; at += align_up((size_t)prefix_off[R] + 16);
    const size_t o_slot = at; at += slot ? align_up((size_t)R * 4 + 4) : 0;
    const size_t o_uk = at; at += slot ? align_up((size_t)R * 2 + 4) : 0;
    for (uint32_t s = 0; s < S; ++s) {
        o_moff[s] = at; at += offs_bytes;
        o_mtext[s] = at; at += align_up((size_t)off[s][R] + 16);
    }
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, at) != hipSuccess) { (void)hipGetLastError(); return PG_ERR_NOMEM; }
    std::vector<RLinesMember> members(S);
    for (uint32_t s = 0; s < S; ++s) { members[s].off = (const uint64_t*)(d + o_moff[s]); members[s].text = (const char*)(d + o_mtext[s]); }
    desc[0].prefix_off = (const uint64_t*)(d + o_poff);
    desc[0].prefix = (const char*)(d + o_pbytes);
    if (slot) { desc[0].slot = (const uint32_t*)(d + o_slot); desc[0].uk = (const uint16_t*)(d + o_uk); }
    bool ok = hipMemcpy(d + L.o_desc, desc.data(), sizeof(RLinesDesc), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + L.o_members, members.data(), (size_t)S * sizeof(RLinesMember), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_poff, prefix_off, ((size_t)R + 1) * 8, hipMemcpyHostToDevice) == hipSuccess &&
              (prefix_off[R] == 0 || hipMemcpy(d + o_pbytes, prefix, prefix_off[R], hipMemcpyHostToDevice) == hipSuccess) &&
              (!slot || (hipMemcpy(d + o_slot, slot, (size_t)R * 4, hipMemcpyHostToDevice) == hipSuccess &&
                         hipMemcpy(d + o_uk, uk, (size_t)R * 2, hipMemcpyHostToDevice) == hipSuccess));
    for (uint32_t s = 0; s < S && ok; ++s)
        ok = hipMemcpy(d + o_moff[s], off[s], ((size_t)R + 1) * 8, hipMemcpyHostToDevice) == hipSuccess &&
             (off[s][R] == 0 || hipMemcpy(d + o_mtext[s], text[s], off[s][R], hipMemcpyHostToDevice) == hipSuccess);
    if (ok) {
        rlines_launch(d, L, slotted, nullptr, 1, blk, eblk, R, bound, nullptr);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
             hipMemcpy(out_off, d + L.o_off, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost) == hipSuccess && out_off[R] <= bound &&
             (out_off[R] == 0 || hipMemcpy(out, d, out_off[R], hipMemcpyDeviceToHost) == hipSuccess);
    }
    hipFree(d);
    return ok ? PG_OK : PG_ERR_DEVICE;
}

}  // namespace

extern "C" int pg_record_lines_from_text(int device, uint64_t n_records, uint64_t n_members, const uint64_t* const* off, const char* const* text,
                                         const uint64_t* prefix_off, const char* prefix, uint64_t* out_off, char* out, uint64_t cap) {
    return rlines_from_text(device, n_records, n_members, off, text, prefix_off, prefix, nullptr, nullptr, false, out_off, out, cap);
}

extern "C" int pg_record_lines_from_text_slotted(int device, uint64_t n_records, uint64_t n_members, const uint64_t* const* off, const char* const* text,
                                                 const uint64_t* prefix_off, const char* prefix, const uint32_t* slot, const uint16_t* uk, uint64_t* out_off,
                                                 char* out, uint64_t cap) {
    return rlines_from_text(device, n_records, n_members, off, text, prefix_off, prefix, slot, uk, true, out_off, out, cap);
}
