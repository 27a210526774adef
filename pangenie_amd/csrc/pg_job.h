// pg_job.h — what the host units of the C-ABI shim share (pg_shim.cpp: jobs, their build and uploads; pg_shim_run.cpp: the
// run schedule, pg_job_run; pg_shim_calls.cpp: the output columns formed from a job's finished bins; pg_shim_lines.cpp: whole VCF lines joined from the record text or the phased text; pg_shim_phase.cpp: the phasing column; pg_shim_panel.cpp: the sampled panel's columns; pg_shim_combine.cpp: path subsets combined): the error helpers, the
// host's picture of a job's index contigs, chains and record plans, struct pg_job itself, and the few helpers upload and run
// both need.  Private: nothing here is exported.
#pragma once
#include <hip/hip_runtime_api.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pangenie_hmm.h"
#include "pg_device.h"
#include "pg_launch.h"

namespace pgj __attribute__((visibility("hidden"))) {

inline void set_err(char* err, size_t errlen, const char* fmt, ...) {
    if (!err || errlen == 0) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, errlen, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(call)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            set_err(err, errlen, "%s failed: %s", #call, hipGetErrorString(e_));          \
            return PG_ERR_DEVICE;                                                         \
        }                                                                                 \
    } while (0)

constexpr int PG_MAX_DEVICES_HOST = 64;
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

struct IndexHost {   // one index contig
    uint32_t V = 0, H = 0, HP = 0, T = 0, RB = 0, part_slots = 2, pair_n = 1;
    bool lean = false;  // every object biallelic and H = HP = 64: the store-only phases run on k_sweep_lean
    bool cls4 = false;  // HP = 16 / 32, H = HP, every object biallelic, fused job: class sums instead of per-thread partials (DevContig::cls4)
    bool leanx = false; // HP = 128 / 64 and every object has at most PG_AMAX alleles (not `lean`): the store-only phases run on k_sweep_leanx
    bool small = false; // every object biallelic and H = HP = 16: the store-only phases run on k_sweep_small16
    bool smallx = false; // H = HP = 16 with multiallelic objects (the 15 + 1 sampled paths): k_sweep_small16x (pg_small16x.h)
    std::vector<uint32_t> list_b;            // ... and k_prep_bi's own
    size_t o_list_b = 0;
    std::vector<uint32_t> list_m4, list_w;   // prep_fast == 2: the objects of k_prep_m4 (3 .. PG_AMAX alleles, <= 64 k-mers) / of k_prep (neither that nor k_prep_bi's)
    size_t o_list_m4 = 0, o_list_w = 0;
    std::vector<uint32_t> auxidx;    // [V] aux slot offset / 16 of every variant with more than two alleles (smallx), PG_WIDE_NONE otherwise
    uint64_t aux_bytes = 0;
    uint32_t n_wide_cand = 0;        // variants with more than PG_AMAX alleles (each may be a wide column)
    bool widef_cand = false, widef = false;   // 64-path chains on the general kernel with such variants: in a fused job a wide column costs that column (DevContig::widef)
    size_t o_auxidx = 0;
    uint32_t prep_fast = 0;  // 1: every object has exactly two alleles and <= 32 k-mers, H <= 64: k_prep_bi; 2: at least half of them (k_prep the rest)
    // The split path (pg_device.h, pg_split.h): 1 / 2 = the chains over this index contig are small / smallx chains whose
    // per-variant work is split into what the index alone decides (formed once per upload) and what the sample's counts decide
    uint32_t split = 0;
    bool all_sb = false;     // every object is k_prep_s_bi's (two alleles, <= 32 k-mers): no lists
    std::vector<uint32_t> list_big;   // variants with more than 32 alleles: the wave-per-object index kernels' list (the others: one thread each)
    size_t o_list_big = 0;
    // index-level device arrays (every chain over this contig points at them)
    size_t o_kept = 0, o_apres = 0, o_colv = 0, o_colof = 0, o_ixpd = 0, o_ixrec = 0, o_ixbin = 0, o_ixwl = 0, o_ixnw = 0;
    uint32_t sumK = 0, sumA = 0;
    uint64_t n_lik = 0, wide_bytes = 0;
    std::vector<uint16_t> n_kmers;   // [V] K of every variant
    std::vector<uint32_t> widx;      // [V] wide entry offset / 16 (only if wide_bytes)
    std::vector<uint64_t> goff;      // [V+1]
    std::vector<uint64_t> pos;       // [V] host copy of the positions (run_phasing: the Viterbi's transition probabilities)
    std::vector<uint32_t> koff, aoff;  // [V+1] the per-variant layout the arena, goff / widx and the kernel choice were planned for
    // device
    size_t o_pos = 0, o_koff = 0, o_aoff = 0, o_aid = 0, o_aflag = 0, o_akoff = 0, o_akmask = 0, o_pa = 0, o_goff = 0, o_widx = 0;
};

struct ChainHost {
    uint32_t index = 0;
    std::vector<uint16_t> coverage;  // [V] host copy (GenotypingResult::set_coverage)
    size_t o_cov = 0, o_kcnt = 0;
    uint64_t lik_first = 0;          // offset of this chain's bins inside the packed lik / lik_exp regions
    DevContig d;
    uint32_t n_cols_host = 0;
};

// One index contig's record plan (pg_record_plan, include/pangenie_hmm.h) as the host keeps it, and its device copy.
struct RecordPlanHost {
    bool set = false;
    uint32_t V = 0, R = 0;
    std::vector<uint32_t> rec_off, rec_var, map_off, vcf_off;
    std::vector<uint16_t> map, vcf_index;
    unsigned char* d = nullptr;   // rec_var, map_off, map, vcf_off, vcf_index: one allocation
    RecPlanDev dev = {};
};
// A plan a job holds: its index contigs refer to it, one alone (pg_job_record_plan) or every member of a stride
// (pg_job_record_plan_strided); the device copy goes with the last reference.
using RecordPlanRef = std::shared_ptr<const RecordPlanHost>;
inline RecordPlanRef record_plan_ref(RecordPlanHost&& h) {
    return RecordPlanRef(new RecordPlanHost(std::move(h)), [](const RecordPlanHost* p) { if (p->d) hipFree(p->d); delete p; });
}

// The record plans' checks and device copies (pg_shim_calls.cpp), shared by the record families of single chains and of
// combined groups.  check_record_plan: everything that needs the plan alone, and the host copy; check_record_plan_ids: every
// allele id of the contig's bubbles has an entry in the map of each of the bubble's records.
int check_record_plan(const pg_record_plan* p, uint32_t V, RecordPlanHost* h, char* err, size_t errlen);
int check_record_plan_ids(const RecordPlanHost& h, const uint32_t* allele_off, const uint16_t* allele_id, char* err, size_t errlen);
size_t record_plan_device_bytes(const RecordPlanHost& h);
bool record_plan_upload(const RecordPlanHost& h, unsigned char* d, RecPlanDev* dev);   // d: record_plan_device_bytes of room
std::vector<uint64_t> record_gl_offsets(const RecordPlanHost& h);                        // [R + 1] first GL value of every record
const RecordPlanHost* plan_of_chain(const pg_job* job, uint32_t c);                      // the plan of chain c's index contig, or nullptr
// k_rplan_ids over the RCallsDesc list of plan_rcalls on the device (d_hit: 8 bytes next to it); passes at once while
// pg_job::rplan_ids_ok
int check_record_plan_ids_on_device(pg_job* job, const RCallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, unsigned char* d_hit, char* err, size_t errlen);

// The wave-per-record kernel stages a bubble's quotients and a record's folded map in device memory: one slot of `stride`
// 16-byte values per block, at most 1024 blocks and 256 MB (a 256-allele bubble: 32 896 bins and as many keys, 1 MB a slot).
struct RcallsLaunch {
    std::vector<uint64_t> first;
    std::vector<RCallsDesc> desc;
    std::vector<uint32_t> wide;   // {descriptor, record} pairs
    uint32_t n_blocks = 0, max_bins = 0, stride = 0, n_slots = 0;
};
// planOf(c): the plan of chain c's index contig or nullptr; aoff(c): the chain's allele_off; per: records per block of the
// lane-per-record kernel.  (pg_shim_combine.cpp plans the records of combined groups with it: a group where this says chain.)
template <class PlanOf, class AoffOf>
void plan_rcalls(uint32_t n_chains, PlanOf planOf, AoffOf aoff, uint32_t per, RcallsLaunch* L) {
    L->first.assign((size_t)n_chains + 1, 0);
    L->desc.clear();
    L->wide.clear();
    uint32_t blk = 0;
    uint64_t max_bins = 0, max_keys = 0;
    for (uint32_t c = 0; c < n_chains; ++c) {
        const RecordPlanHost* h = planOf(c);
        const uint32_t R = h ? h->R : 0;
        L->first[c + 1] = L->first[c] + R;
        if (R == 0) continue;
        RCallsDesc d;
        memset(&d, 0, sizeof(d));
        d.blk0 = blk; d.R = R; d.chain = c;
        d.plan = h->dev;
        const uint32_t* off = aoff(c);
        for (uint32_t v = 0; v < h->V; ++v) {
            const uint64_t A = off[v + 1] - off[v];
            if (A <= PG_AMAX) continue;
            for (uint32_t q = h->rec_off[v]; q < h->rec_off[v + 1]; ++q) {
                const uint64_t nA = h->vcf_off[q + 1] - h->vcf_off[q];
                L->wide.push_back((uint32_t)L->desc.size());
                L->wide.push_back(q);
                max_bins = std::max(max_bins, A * (A + 1) / 2);
                max_keys = std::max(max_keys, nA * (nA + 1) / 2);
            }
        }
        L->desc.push_back(d);
        blk += (R + per - 1) / per;
    }
    L->n_blocks = blk;
    L->max_bins = (uint32_t)max_bins;
    L->stride = (uint32_t)(max_bins + max_keys);
    const uint64_t n_wide = L->wide.size() / 2;
    L->n_slots = n_wide ? (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n_wide, 1024), std::max<uint64_t>(1, ((uint64_t)256 << 20) / ((uint64_t)L->stride * 16))) : 0;
}

// What a job keeps of ONE output family (the calls, the record calls, the record GLs; pg_shim_calls.cpp): a device buffer of its
// own outside the arena — the output chain after chain, then (record GLs: the plans' offsets, then) the chain descriptors, the
// wide kernel's list and its staging slots — and what a launch over it needs.  Made by the family's first forming (a job whose
// user fetches bins never pays for it), freed in pg_job_destroy.
struct OutputFamily {
    unsigned char* d = nullptr;
    std::vector<uint64_t> first;              // [n_chains + 1] first element of every chain (a chain without variants / a plan has none)
    size_t o_desc = 0, o_wide = 0, o_stage = 0;   // bytes into d: descriptors, the wide list, the staging slots (records only)
    uint32_t blocks = 0, wide = 0, max_bins = 0, stride = 0, slots = 0;
    bool dirty = true;                        // records: a plan or the index changed: descriptors, lists and the id check are redone
    bool formed = false;                      // a launch over the buffer as it is has finished (NOT reset by a later pg_job_run)
    uint64_t run = 0;                         // pg_job::run_serial of the run that launch formed it from (0: none)
    double ms = 0.0;
    void release() { if (d) hipFree(d); d = nullptr; }
};

// The record text (pg_job_record_text) is one more family: `first` = the first RECORD of every chain, and d =
// the packed text, then every record's first byte in it (64 bits, one more behind the last), the scan's arrays, the
// descriptors and the wide list.  Unlike its siblings it is stale after a later run: its fetches ask for `run`.
struct RecordTextFamily : OutputFamily {
    std::vector<uint64_t> text_first;         // [n_chains + 1] first byte of every chain (after a forming)
    std::vector<RTextDesc> desc;              // host copy (chains with records)
    size_t o_off = 0, o_loc = 0, o_wlen = 0, o_bsum = 0, o_bbase = 0;
    size_t o_uk = 0;                          // the panel text alone: [n_records] 16-bit UK of every record, for slotted lines over it (0: none)
    uint64_t n_records = 0, cap = 0;
    uint64_t serial = 0;                      // counts the finished formings: the record lines remember which text they joined
    hipEvent_t ev_emit[2];
    bool events = false;
    double emit_ms = 0.0;
    void release() {
        OutputFamily::release();
        if (events) { hipEventDestroy(ev_emit[0]); hipEventDestroy(ev_emit[1]); events = false; }
    }
};

// The record lines (pg_job_record_lines) are the family above the text: per index contig that has a plan, a
// prefix and members, the line of every record — the caller's prefix, every member's text, a newline — packed.  d = the
// packed lines (the exact bound), then every line's first byte (64 bits, one more behind the last), the scan's arrays, the
// descriptors and the members.  A prefix is a device buffer of its own: [R + 1] offsets, then (a slotted one, DESIGN.md
// 4e-8) [R] slots, then the bytes.  Index contigs refer to it, one alone (pg_job_line_prefix[_slotted]) or every member of a
// stride (pg_job_line_prefix_strided); the buffer goes with the last reference, as a record plan's does.
// Stale when the text it joined is stale or formed anew, and when a prefix changed.
struct LinePrefix {
    unsigned char* d = nullptr;
    uint32_t R = 0;
    uint64_t bytes = 0;
    size_t o_slot = 0, o_bytes = 0;           // bytes into d: the slots (0: a plain prefix), the prefix bytes
};
using LinePrefixRef = std::shared_ptr<const LinePrefix>;
inline LinePrefixRef line_prefix_ref(const LinePrefix& p) {
    return LinePrefixRef(new LinePrefix(p), [](const LinePrefix* q) { if (q->d) hipFree(q->d); delete q; });
}
struct RecordLinesFamily : OutputFamily {
    std::vector<LinePrefixRef> prefix;        // [n_index] (sized by the first pg_job_line_prefix*); null: none
    std::vector<uint64_t> line_first, byte_first;   // [n_index + 1] first line / first byte of every index contig (after a forming)
    size_t o_off = 0, alloc = 0;
    uint64_t n_lines = 0, cap = 0;
    uint64_t text_serial = 0;                 // RecordTextFamily::serial of the text the lines were joined from
    void drop_prefix(size_t ix) {
        if (ix < prefix.size() && prefix[ix]) { prefix[ix].reset(); formed = false; }
    }
    void release() {
        OutputFamily::release();
        for (size_t ix = 0; ix < prefix.size(); ++ix) drop_prefix(ix);
        alloc = 0;
        formed = false;
    }
};

// What a job keeps of its combine plan (pg_shim_combine.cpp): the groups, and ONE device buffer outside the
// arena — the combined bins group after group, the calls, then the group descriptors, the member list, the wide kernels' list,
// the pairs of the layout check and its word.  A second plan makes a new one.
struct CombineState {
    bool planned = false;
    bool layout_ok = false;                    // k_combine_check has passed the members' layouts as the device holds them
    std::vector<uint32_t> group_off, members;  // [n_groups + 1], [group_off[n_groups]]: chains in combine order
    std::vector<uint64_t> bin_first, var_first;   // [n_groups + 1] first bin / first variant of every group
    std::vector<CombineDesc> desc;             // host copy (groups with variants)
    std::vector<CombinePair> pairs;
    unsigned char* d = nullptr;
    size_t o_calls = 0, o_desc = 0, o_members = 0, o_wide = 0, o_pairs = 0, o_hit = 0;
    uint32_t blocks = 0, wide = 0, check_items = 0;
    uint64_t combined_run = 0, calls_run = 0;  // pg_job::run_serial of the run they were formed from (0: none)
    hipEvent_t ev[2];
    bool events = false;
    double ms = 0.0, calls_ms = 0.0;
    void release() {
        if (d) hipFree(d);
        d = nullptr;
        if (events) { hipEventDestroy(ev[0]); hipEventDestroy(ev[1]); events = false; }
        planned = false;
    }
};

// What a job keeps of the records of its combined groups (pg_shim_combine.cpp): ONE device buffer outside the
// arena — one pg_call per record group after group, the GL values, the plans' GL offsets, the group descriptors, the wide
// kernels' list, their staging slots (the two formations block, so they share them) and the word of the id check.  Made by the
// first formation, made anew when `dirty`: a record plan, the combine plan or the index changed.
struct CombinedRecordsState {
    unsigned char* d = nullptr;
    std::vector<uint64_t> rec_first, gl_first;   // [n_groups + 1] first record / first GL value of every group (a group without a plan has none)
    std::vector<CRecDesc> desc;                  // host copy (groups with records)
    size_t o_gl = 0, o_desc = 0, o_wide = 0, o_stage = 0, o_hit = 0;
    uint32_t blocks = 0, wide = 0, max_bins = 0, stride = 0, slots = 0;
    bool dirty = true;
    // pg_job::combine_serial of the pg_job_combine whose bins the ids were checked beside / the records / the values were formed from (0: none)
    uint64_t ids_serial = 0, calls_serial = 0, gl_serial = 0;
    double calls_ms = 0.0, gl_ms = 0.0;
    void release() { if (d) hipFree(d); d = nullptr; dirty = true; }
};

// The genotype-quality thresholds on `device` (pg_shim_calls.cpp: built once from log10l, uploaded once per device; the
// caller has made `device` current).
int gq_table_on(int device, const uint64_t** d_m, const int32_t** d_e, char* err, size_t errlen);

}  // namespace pgj

struct pg_job {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<pgj::IndexHost> index;
    std::vector<pgj::ChainHost> chains;
    uint32_t n_contigs = 0, n_samples = 1;  // chains = n_samples * n_contigs (sample-major)
    bool cohort = false;
    DevContig* d_contigs = nullptr;
    unsigned char* arena = nullptr;
    size_t arena_bytes = 0;
    bool cache_arena = false;  // hand the arena to the process cache on destroy (one-shot call)
    // regions zeroed at the start of every run
    unsigned char* zero_base = nullptr;
    size_t zero_bytes = 0;
    uint32_t* d_small = nullptr;  // [n_small] chain ids of the H = 16 chains
    uint32_t n_small = 0;
    uint32_t* d_smallx = nullptr; // [n_smallx] ... of those with multiallelic objects (k_sweep_small16x), behind d_small's
    uint32_t n_smallx = 0;
    bool smallx_phase2 = false;
    bool small_phase2 = false;    // some of them (fused jobs, class sums: DevContig::small == 2) also run their phase 2 on k_sweep_small16
    double* d_dump = nullptr;
    uint32_t* d_ncols = nullptr;  // [n_index] kept columns of every index contig (k_compact, when the index is uploaded)
    uint32_t* d_ixerr = nullptr;  // [n_index] error bits of the index-level kernels
    DevContig* d_reps = nullptr;  // [n_index] one chain descriptor per index contig: what the index-level kernels walk
    unsigned char* ix_base = nullptr;   // the index-derived arrays of all contigs, one run of the arena (zeroed before every index pass)
    size_t ix_bytes = 0;
    unsigned char* srec_base = nullptr; // the sample records of all split chains, one run (zeroed with every index pass: k_prep_s_bi leaves the zero pieces out)
    size_t srec_bytes = 0;
    bool any_split = false;
    uint32_t max_sb = 0, max_sm4 = 0, max_sw = 0;   // grid extents of the split path's emission kernels
    bool any_legacy_prep = false;
    hipEvent_t ev_ix[2];
    double index_ms = 0.0;
    std::string plan_text;
    std::vector<unsigned char> tab_p;
    size_t o_tab_p = 0;
    uint32_t* d_err = nullptr;    // [n_chains]
    double* d_lik = nullptr;      // packed, chain after chain
    int32_t* d_likexp = nullptr;
    uint64_t n_lik_total = 0;
    size_t o_tab_m = 0, o_tab_e = 0;
    std::vector<double> tab_m;
    std::vector<int32_t> tab_e;
    DevTable tab;
    uint32_t hp_mask = 0, max_v = 0;   // hp_mask: the PG_SWEEP_* bits of the job's chain kernels (pg_launch.h; choose_chain_kernels)
    uint32_t max_wide = 0;   // grid extent of k_bins_wide: the longest list of wide-column candidates
    uint32_t max_prep_w = 0, max_prep_m4 = 0;   // grid extents of k_prep (lists or all variants) and k_prep_m4
    uint32_t bins_which = 0;   // the PG_BINS_* bits of the kernels that form a fused job's bins
    uint32_t vit_bits = 0;     // run_phasing: 1 / 2 / 4 = chains with 16 / 32 / 64 padded paths
    hipEvent_t ev_vit[2];
    double vit_ms = 0.0;
    bool vit_tq_ready = false;  // the transition probabilities of the kept columns are on the device (they depend on the index only)
    hipEvent_t ev[PG_N_KERNEL_CLASSES + 1];
    bool events = false;
    double ms[PG_N_KERNEL_CLASSES] = {0, 0, 0, 0, 0, 0};
    double host_s[4] = {0, 0, 0, 0};
    uint64_t up_bytes[2] = {0, 0};
    pg_hmm_params params;
    bool ran = false;
    uint64_t run_serial = 0;   // counts the finished pg_job_run calls: what was formed from a run's bins remembers which
    // Sweep mode.  fused: phase 2 forms the posterior partials inline (k_bins reduces them) — least
    // HBM traffic, the choice when hundreds of chains fill the chip.  chunked: with few chains the
    // chip is idle and a chain's time is its per-column latency, so phase 2 runs as store-only
    // chunks (as cheap per column as phase 1) and k_post forms the posteriors of each finished
    // chunk on the idle CUs from a second stream.
    bool chunked = false;
    uint32_t chunk_cols = 0, n_chunks = 0;
    // chunked jobs whose chains are ALL lean chains, few enough that every workgroup of k_sweep_lean<4> and k_post_loop has a CU
    // of its own: phase 2 is ONE launch of each, chunks handed over through DevContig::sync (PG_KERNELS=nopersist: a launch per chunk)
    bool persist = false;
    uint32_t post_blocks = 0;
    // chunked jobs (a launch per chunk) that leave CUs idle, chunk_cols a multiple of PG_LEAN_SPARSE: phase 1 of the lean chains stores
    // only its checkpoints and k_refill_lean forms the columns between them on the second stream, chunk by chunk in front of k_post
    // (DevContig::sparse; PG_KERNELS=nosparse: every column by the chain)
    bool sparse = false;
    // ... and every chain with columns is such a chain: the chunk sweeps of phase 2 store only their checkpoints too, into an area
    // of their own (DevContig::sparse2), and k_refill_lean forms each chunk's columns behind its sweep on the second stream — which
    // then owns the scratch buffers alone: the sweeps wait for no k_post (PG_KERNELS=nosparse2: dense chunk sweeps)
    bool sparse2 = false;
    std::vector<hipEvent_t> ev_chunk;   // sparse2: one "sweep done" event per chunk (the sweeps run chunks ahead of the stream that waits for them)
    // sparse2 jobs of more than one piece: phase 1 runs as one launch per piece of `piece_chunks` partner chunks (pg_device.h:
    // pg_sparse_piece), the farthest from the phase boundary first, and the second stream — idle in phase 1 — refills the partner
    // columns of a piece's chunks behind it, beside the pieces that follow.  Only piece 0's chunks are left for phase 2 to refill.
    // (PG_KERNELS=nopieces: one launch; PG_PIECE_CHUNKS: chunks per piece.)  n_pieces == 1: the single launch
    uint32_t piece_chunks = 0, n_pieces = 1;
    uint32_t piece_refill_blocks = 0;   // workgroups of a refill launched beside phase 1: fewer than in phase 2 (job_build)
    std::vector<hipEvent_t> ev_piece;   // one "piece done" event per piece
    // ... whose chains are all k_prep_bi's (no k_prep, k_prep_m4, no lists, no split chains), n_pieces >= prep_early + 1: a run on
    // the job's own stream prepares only the ENDS of the chains — what the first prep_early pieces read — ahead of phase 1, and the
    // MIDDLE (pg_device.h: pg_prep_middle, half-width prep_W columns) on the second stream beside those pieces; `s` waits for
    // ev_prep2 in front of piece n_pieces - prep_early - 1 (pg_shim_run.cpp: prepare_in_parts, phase1_in_pieces).
    // (PG_KERNELS=prepahead: the whole preparation ahead; PG_PREP_EARLY_PIECES: prep_early.)
    bool prep_beside = false;
    uint32_t prep_early = 0, prep_W = 0;
    // the grid extents of the two parts: the most variants / columns a chain has in part 1 ([0]) and in part 2 ([1]) — read off the
    // column lists on the device by the first such run behind an index upload
    bool prep_parts_ready = false;
    uint32_t prep_max_v[2] = {0, 0}, prep_max_c[2] = {0, 0};
    hipEvent_t ev_prep2 = nullptr;
    // The pipelined first run of a one-shot job (job_build with cache_arena: upload and run inside ONE call, the host arrays stay
    // valid): the inputs of the LONG chains (group A: the job's wall time) are uploaded first and their preparation + phase 1
    // start while the other chains' inputs (group B, most of the bytes) are still crossing PCIe; B's index pass, preparation and
    // phase 1 then run on the second stream beside A's.  24 chromosomes x 64 paths: 27 ms of H2D in front of a 252 ms run.
    bool pipeline = false, pipeline_capable = false, late_pending = false;
    uint32_t nA = 0;
    std::vector<uint32_t> grp_order;          // chains (= index contigs: 1:1 in such jobs), group A first
    DevContig* d_contigs_g = nullptr;         // the chain descriptors in that order
    DevContig* d_reps_g = nullptr;            // the index descriptors in that order
    std::vector<std::thread> late_threads;    // group B's copies
    std::vector<int> late_rc;
    hipEvent_t ev_late[2];
    bool ev_late_made = false;
    hipStream_t persist_checked = nullptr;   // the stream whose kernels are known to run beside stream2's (streams_concurrent)
    bool persist_checked_any = false;
    uint32_t* d_handshake = nullptr;
    uint32_t persist_runs = 0, persist_fallbacks = 0;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_sweep[PG_SCRATCH_BUFS], ev_post[PG_SCRATCH_BUFS];
    bool events2 = false;
    // Per-sample inputs (read k-mer counts, local coverage) of all chains lie in ONE contiguous run of the arena,
    // [sample_lo, sample_lo + sample_bytes): a cohort's next batch of samples is packed by host threads into a pinned
    // staging buffer of the same layout and moved with a handful of large copies (sample_upload) — and, through
    // pg_job_upload_begin / _end, into a SECOND set of arrays while the current one is being genotyped.
    size_t sample_lo = 0, sample_bytes = 0;
    unsigned char* staging = nullptr;         // pinned, sample_bytes (allocated on first use)
    bool staging_refused = false;             // hipHostMalloc failed once: sample uploads copy chain by chain from pageable memory
    unsigned char* alt_samples = nullptr;     // device: the other set of per-sample arrays (allocated on first pg_job_upload_begin)
    DevContig* d_contigs_alt = nullptr;       // chain descriptors pointing into the other set (the spare of the two descriptor arrays)
    DevContig* d_contigs_owned = nullptr;     // the descriptor array that is not part of the arena (to free)
    std::vector<DevContig> h_contigs;         // host copy of the descriptors of the set in use
    unsigned char* cur_samples = nullptr;     // base of the set in use (arena + sample_lo, or alt_samples)
    hipStream_t copy_stream = nullptr;
    std::thread uploader;                     // pg_job_upload_begin's worker
    bool upload_pending = false;
    int upload_rc = PG_OK;
    std::string upload_err;
    std::vector<std::vector<uint16_t>> next_coverage;   // host copies of the pending batch's coverage arrays
    hipEvent_t ev_fill = nullptr;             // orders a count plan's stream against the job's (pgi_job_fill_begin / _end; made by the first fill)
    // The output columns formed from the finished bins (pg_shim_calls.cpp), one OutputFamily each; the host copies of the
    // descriptors keep their own types.  Calls (pg_job_calls): one 8-byte record per variant, chain after chain.
    pgj::OutputFamily calls;
    std::vector<CallsDesc> calls_desc;        // host copy of the descriptors (chains with variants)
    hipEvent_t ev_calls[2];                   // the three families time their launches with the same two events
    bool calls_events = false;
    // Record calls (pg_job_record_plan / pg_job_record_calls): one plan per index contig, shared by every chain over it, and one
    // 8-byte record per VCF record of every chain whose index contig has a plan.
    std::vector<pgj::RecordPlanRef> rplans;   // [n_index] (sized by the first pg_job_record_plan[_strided]); null: no plan
    bool rplan_ids_ok = false;                // k_rplan_ids has passed the plans and the index as they are
    pgj::OutputFamily rcalls;
    std::vector<RCallsDesc> rcalls_desc;
    // Record GLs (pg_job_record_gl): 4 bytes per genotype of every record's defined alleles, chain after chain, under the same plans.
    pgj::OutputFamily rgl;                    // (first: the first VALUE of every chain)
    std::vector<RGlDesc> rgl_desc;
    // Record text (pg_job_record_text): the bytes of the GT:GQ:GL:KC column of every record, packed, from the two families above.
    pgj::RecordTextFamily rtext;
    // Record lines (pg_job_line_prefix / pg_job_record_lines): whole VCF lines per index contig, every member's text joined in.
    pgj::RecordLinesFamily rlines;
    // The phasing column of a run_phasing job (pg_shim_phase.cpp), under the same plans: two numbers per VCF
    // record from the Viterbi haplotypes (pg_job_record_phase), the bytes of `GT:KC` from them (pg_job_phased_text: a
    // RecordTextFamily without wide records) and whole lines over prefixes of their own (pg_job_phased_lines).  All three are
    // stale after a later run.
    pgj::OutputFamily rphase;
    std::vector<RPhaseDesc> rphase_desc;
    pgj::RecordTextFamily ptext;
    std::vector<PTextDesc> ptext_desc;
    pgj::RecordLinesFamily plines;
    // The sample columns of the sampled-panel VCF (pg_shim_panel.cpp), under the same plans: the bytes of
    // every record's P cells from the chain's reduced panel (pg_job_panel_text: a RecordTextFamily that no run makes stale —
    // it reads the panel, not the bins) and whole lines over `GT` prefixes of their own (pg_job_panel_lines), whose UK is
    // the panel's own count, kept per record next to the text.
    pgj::RecordTextFamily paneltext;
    std::vector<PanelDesc> panel_desc;
    pgj::RecordLinesFamily panellines;
    // Path subsets combined on the device (pg_job_combine_plan / pg_job_combine / pg_job_combined_calls).
    pgj::CombineState combine;
    uint64_t combine_serial = 0;              // counts the finished pg_job_combine calls
    // ... and GT, GQ and GL per VCF record of the combined groups (pg_job_combined_record_calls / pg_job_combined_record_gl).
    pgj::CombinedRecordsState crec;
};

namespace pgj __attribute__((visibility("hidden"))) {

// a plan was set or the index uploaded anew (new allele ids): both record families rebuild and the ids are checked again
inline void record_plans_changed(pg_job* job) {
    job->rcalls.dirty = true;
    job->rgl.dirty = true;
    job->rtext.dirty = true;          // (its descriptors point into the two buffers above)
    job->rphase.dirty = true;         // (the phasing column: its descriptors hold the plans' device arrays)
    job->ptext.dirty = true;
    job->paneltext.dirty = true;      // (the panel text: the plans' arrays, and with a new index a new panel)
    job->rplan_ids_ok = false;
    job->combine.layout_ok = false;   // (the members' layouts are compared again before the next combine)
    job->crec.dirty = true;           // (the records of the combined groups: rebuilt, the ids checked again)
}

// The three text families of a job and the lines joined from each.  What the fetches of a text (pg_shim_calls.cpp) and the
// whole of the lines (pg_shim_lines.cpp) do is written once and told the family by one of these rows; the formers differ.
struct TextKind {
    RecordTextFamily pg_job::*text;
    const char* former;   // the entry point that forms it, as the messages name it
    bool per_run;         // formed from a run's results: stale after the next run, nothing without one (the panel text is neither)
};
struct LinesKind {
    TextKind text;
    RecordLinesFamily pg_job::*lines;
    const char* former;
};
inline const TextKind kRecordText = {&pg_job::rtext, "pg_job_record_text", true};
inline const TextKind kPhasedText = {&pg_job::ptext, "pg_job_phased_text", true};
inline const TextKind kPanelText = {&pg_job::paneltext, "pg_job_panel_text", false};
inline const LinesKind kRecordLines = {kRecordText, &pg_job::rlines, "pg_job_record_lines"};
inline const LinesKind kPhasedLines = {kPhasedText, &pg_job::plines, "pg_job_phased_lines"};
inline const LinesKind kPanelLines = {kPanelText, &pg_job::panellines, "pg_job_panel_lines"};
// formed for the last run and the plans as they are?  then: every chain's first byte; one chain's bytes and offsets; all
// chains' from one copy; one chain's device pointers
int text_family_ready(pg_job* job, const TextKind& k, char* err, size_t errlen);
int text_family_first(pg_job* job, const TextKind& k, uint64_t* text_first, char* err, size_t errlen);
int text_family_fetch_chain(pg_job* job, const TextKind& k, uint32_t ci, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int text_family_fetch_packed(pg_job* job, const TextKind& k, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int text_family_device(pg_job* job, const TextKind& k, uint32_t ci, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes);

// Group B's copies of a pipelined first run (pg_job::late_threads) read the caller's arrays and feed the job's second stream:
// whoever needs either to be left alone waits for the threads first.
inline void join_late_threads(pg_job* job) {
    for (auto& t : job->late_threads) if (t.joinable()) t.join();
    job->late_threads.clear();
    job->late_pending = false;
}

// grid extent of the wave-per-object index kernels (pgk_launch_index): the longest list of variants with more than 32 alleles
inline uint32_t max_big_list(const pg_job* job) {
    uint32_t max_big = 0;
    for (const IndexHost& x : job->index) if (x.list_big.size() > max_big) max_big = (uint32_t)x.list_big.size();
    return max_big;
}

// Do the kernels of `s` and of the job's second stream run side by side?  (pg_shim_run.cpp; upload_inputs asks for the pipelined
// first run, pg_job_run for the persistent phase 2.)  May replace job->stream2.
bool streams_concurrent(pg_job* job, hipStream_t s);

}  // namespace pgj
