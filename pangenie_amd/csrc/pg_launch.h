// pg_launch.h — the launch seam between the C-ABI shim (pg_shim.cpp, pg_shim_run.cpp, pg_shim_calls.cpp, pg_shim_phase.cpp, pg_shim_panel.cpp) and the kernels (pg_kernels.hip, pg_viterbi.hip, pg_calls.hip, pg_combine.hip, pg_combine_records.hip, pg_record_text.hip, pg_record_lines.hip, pg_phase_text.hip, pg_panel_text.hip).
//
// The ONE declaration of every host-callable launcher and of the two launch masks a job hands them.  Both sides include
// it: a launcher whose parameter list changes on one side only no longer compiles (C linkage: the linker would not notice).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "pg_device.h"

// Sweep mask (pg_job::hp_mask -> pgk_launch_sweep / pgk_launch_sweep_chunk): which chain kernels a job's sweep launches.
// Every kernel walks all chains of the job and returns at once for a chain that is not its own.
enum : uint32_t {
    PG_SWEEP_HP16 = 1u,            // k_sweep<16,4>: the general kernel, one bit per padded path count
    PG_SWEEP_HP32 = 2u,            // k_sweep<32,8>
    PG_SWEEP_HP64 = 4u,            // k_sweep<64,16>
    PG_SWEEP_HP128 = 8u,           // k_sweep<128,32>
    PG_SWEEP_GENERIC = 16u,        // k_sweep_generic: chains with HP >= 256
    PG_SWEEP_GENERIC64 = 32u,      // (forced, PG_KERNELS=generic) ... for every HP >= 64; goes with PG_SWEEP_GENERIC: one launch covers both
    PG_SWEEP_LEAN = 64u,           // k_sweep_lean: lean chains (all-biallelic, H = HP = 64), the store-only phases
    PG_SWEEP_TRI = 128u,           // fused job whose 64-path chains store triangles (DevContig::tri): phase 1 of the lean chains on k_sweep_lean_tri
    PG_SWEEP_LEAN2 = 256u,         // k_sweep_lean2: phase 2 of the chains with tri == 2
    PG_SWEEP_LEANX128 = 512u,      // k_sweep_leanx<., 128>: lean-x chains at HP = 128 (narrow columns only)
    PG_SWEEP_LEANX64 = 1024u,      // k_sweep_leanx<., 64>: ... at HP = 64 (chains with multiallelic objects; all-biallelic ones are PG_SWEEP_LEAN's)
    PG_SWEEP_TRI1 = 2048u,         // k_sweep_tri1: 64-path triangle chains that are not lean chains, phase 1 on the general kernel (PG_KERNELS=noleanx)
    PG_SWEEP_LEANX_TRI = 4096u,    // k_sweep_leanx_tri: ... on the lean-x step (DevContig::leanx == 2)
    PG_SWEEP_LEANX2 = 8192u,       // k_sweep_leanx2: phase 2 of the chains with DevContig::leanx2
    PG_SWEEP_LEANX_TRIW = 16384u,  // k_sweep_leanx_triw: phase 1 of those triangle chains that have wide columns (DevContig::widef)
};

// Bins mask (pg_job::bins_which -> pgk_launch_bins): which kernels form a fused job's bins.
enum : uint32_t {
    PG_BINS_FULL = 1u,     // k_bins has chains of its own (it is launched either way: one block per chain without this bit)
    PG_BINS_LEAN2 = 2u,    // k_bins_lean2: chains on k_sweep_lean2, and class sums (DevContig::cls4)
    PG_BINS_THIN = 4u,     // k_bins_thin: at most 64 partial entries per column
    PG_BINS_X = 8u,        // k_bins_x: chains on k_sweep_small16x<2>
    PG_BINS_WIDE = 16u,    // k_bins_wide: ... with objects of more than PG_AMAX alleles, and DevContig::widef chains: one wave per listed wide column
    PG_BINS_S = 32u,       // k_bins_s: split chains (pg_split.h)
    PG_BINS_WIDE_S = 64u,  // k_bins_wide_s: ... with wide columns
    PG_BINS_Q = 128u,      // k_bins_q: chains on k_sweep_leanx2
};

// Calls (pg_calls.hip): one descriptor per chain that has variants, in chain order.  Blocks [blk0, next blk0) of k_calls take
// pgk_calls_block() variants of the chain each; `out` = the chain's 8-byte records (pg_call, include/pangenie_hmm.h).
struct CallsDesc {
    uint32_t blk0, V;
    uint32_t chain, pad;   // index into the DevContig array
    void* out;
};

// Record calls (pg_calls.hip, k_rcalls / k_rcalls_wide): an index contig's record plan as the device holds it, shared by every
// chain over that contig, and one descriptor per chain that has a plan and variants.  Blocks [blk0, next blk0) of k_rcalls take
// pgk_calls_block() RECORDS of the chain each; `out` = the chain's 8-byte records, one per VCF record.
struct RecPlanDev {
    const uint32_t* rec_var;    // [R] the bubble (variant) of record r; bit 31: the record has alleles of undefined sequence
    const uint32_t* map_off;    // [R+1]
    const uint16_t* map;        // map[map_off[r] + allele id] = the record allele that bubble allele carries
    const uint32_t* vcf_off;    // [R+1]; vcf_off[r + 1] - vcf_off[r] = the record's alleles (at most PG_MAX_ALLELES_PER_VARIANT)
    const uint16_t* vcf_index;  // per record allele: its index among the defined ones, 0xFFFF if its sequence is undefined
};
struct RCallsDesc {
    uint32_t blk0, R;
    uint32_t chain, pad;
    void* out;
    RecPlanDev plan;
};

// Record GLs (pg_calls.hip, k_rgl / k_rgl_wide): as RCallsDesc; `out` = the chain's 4-byte values (pg_gl), record r's at
// gl_off[r] .. gl_off[r + 1] (the offsets hang on the plan alone: one array per index contig)
struct RGlDesc {
    uint32_t blk0, R;
    uint32_t chain, pad;
    void* out;
    const uint64_t* gl_off;
    RecPlanDev plan;
};

// Combined groups (pg_combine.hip): one descriptor per group that has variants, in group order.  The chains of a
// group — members[first .. first + S), indices into the DevContig array in combine order — share one layout (allele_off,
// allele_id, geno_off: read from the first).  Blocks [blk0, next blk0) of k_combine and of k_ccalls take pgk_combine_block()
// variants of the group each; `bins` = the group's 16-byte combined bins (pg_combined_bin [geno_off[V]]), `calls` = its
// 8-byte records (pg_call [V]).
struct CombineDesc {
    uint32_t blk0, V;
    uint32_t first, S;
    void* bins;
    void* calls;
};
// The layout check (k_combine_check): member `member` against the first chain of its group, `ref`; both hold V + 1 offsets
// and sumA allele ids.
struct CombinePair {
    uint32_t ref, member, V, sumA;
};

// Records of combined groups (pg_combine_records.hip): one descriptor per group whose first chain's index
// contig has a record plan with records, in group order.  Blocks [blk0, next blk0) of k_crcalls / k_crgl take
// pgk_combined_records_block() RECORDS of the group each.  The layout (allele_off, allele_id, geno_off) is read from `chain`,
// the group's first; `bins` = the group's combined bins, `calls` = one pg_call per record, `gl` = the group's pg_gl values,
// record r's at gl_off[r] .. gl_off[r + 1].
struct CRecDesc {
    uint32_t blk0, R;
    uint32_t chain, group;
    const void* bins;
    void* calls;
    void* gl;
    const uint64_t* gl_off;
    RecPlanDev plan;
};

// Record text (pg_record_text.hip): one descriptor per chain (or per call of the unit entry point) that has
// records, in chain order.  Blocks [blk0, next blk0) take pgk_rtext_block() RECORDS each; rec0 = the chain's first record
// among all records of the launch (the offsets and the packed text are the launch's, not the chain's).  `calls` = the chain's
// pg_call records, `gl` its pg_gl values, record r's at gl_off[r] .. gl_off[r + 1].  With rec_var (a job's chain): KC, UK and
// the column count are read from DevContig `chain`, under pg_job_fetch's rule; without (the unit entry point): kc [R] and
// no_call [R] (or null) per record.
struct RTextDesc {
    uint32_t blk0, R;
    uint64_t rec0;
    uint32_t chain, ignore_imputed;
    const void* calls;
    const void* gl;
    const uint64_t* gl_off;
    const uint32_t* rec_var;
    const uint16_t* kc;
    const uint8_t* no_call;
};

// Record lines (pg_record_lines.hip): one descriptor per index contig that takes part, in contig order,
// and one RLinesMember per member of each, members[mem0 .. mem0 + S) in member order: record r's text = text[off[r] .. off[r + 1]).
// Blocks [blk0, next blk0) of k_rlines_len take pgk_rlines_block() LINES of the contig each; workgroups [eblk0, next eblk0)
// of k_rlines_emit take lpw = pgk_rlines_lines_per_wave(S, slotted) lines each, `slotted` the launch's.  line0 = the contig's
// first line among all lines of the launch (the offsets and the packed bytes are the launch's).  prefix r =
// prefix[prefix_off[r] .. prefix_off[r + 1]).  The fields from `slot` on are read by a slotted launch alone: where the UK of
// every record goes and comes from.  slot null: a plain prefix.  Otherwise record r's digits stand in front of byte slot[r]
// of its prefix; UK = uk[r] (the unit entry point), or without `uk` the k-mer count of bubble rec_var[r] of DevContig `chain`,
// the contig's first member, under pg_job_fetch's rule.
struct RLinesMember {
    const uint64_t* off;
    const char* text;
};
struct RLinesDesc {
    uint32_t blk0, R;
    uint32_t eblk0, lpw;
    uint64_t line0;
    uint32_t mem0, S;
    const uint64_t* prefix_off;
    const char* prefix;
    const uint32_t* slot;
    const uint16_t* uk;
    const uint32_t* rec_var;
    uint32_t chain, pad;
};

// Record phase and phased text (pg_phase_text.hip): one descriptor per chain (or per call of a unit entry
// point) that has records, in chain order.  Blocks [blk0, next blk0) take pgk_ptext_block() RECORDS each.
// RPhaseDesc: `out` = the chain's 4-byte records (pg_phase, pg_phase.h), one per VCF record.  With hap1 (the unit entry
// point): hap1 / hap2 [V] the haplotypes' allele ids and keyed [V] per variant; without (a job's chain): hap1, hap2 and kept
// of DevContig `chain`, keyed = run_genotyping && kept.
struct RPhaseDesc {
    uint32_t blk0, R;
    uint32_t chain, run_genotyping;
    void* out;
    RecPlanDev plan;
    const uint16_t* hap1;
    const uint16_t* hap2;
    const uint8_t* keyed;
};
// PTextDesc: rec0 = the chain's first record among all records of the launch (the offsets and the packed text are the
// launch's); `phase` = the chain's pg_phase records.  With rec_var (a job's chain): KC and UK are read from DevContig `chain`
// under pg_job_fetch's rule — every bubble's with run_genotyping and a column, else those of the bubbles below the column
// count and 0 beyond; without (the unit entry point): kc [R] and no_call [R] (or null) per record.
struct PTextDesc {
    uint32_t blk0, R;
    uint64_t rec0;
    uint32_t chain, ignore_imputed;
    uint32_t run_genotyping, pad;
    const void* phase;
    const uint32_t* rec_var;
    const uint16_t* kc;
    const uint8_t* no_call;
};

// Panel text (pg_panel_text.hip): one descriptor per chain (or per call of the unit entry point) that has
// records, in chain order.  Blocks [blk0, next blk0) take pgk_ptpanel_block() CELLS of the chain each, cell r P + p = path p
// of record r; rec0 = the chain's first record among all records of the launch (the offsets and the packed text are the
// launch's).  path_allele [V x P] = the chain's reduced panel.  With kmer_off (a job's chain): uk [R] takes the panel's own
// count of every record's bubble (RLinesDesc::uk of the lines over this text); without (the unit entry point): no UK.
struct PanelDesc {
    uint32_t blk0, R;
    uint64_t rec0;
    uint32_t chain, P;
    const uint16_t* path_allele;
    const uint32_t* kmer_off;
    uint16_t* uk;
    RecPlanDev plan;
};

extern "C" {
// pg_panel_text.hip: d_bsum [n_blocks], d_bbase [n_blocks + 1]: the scan's; d_off [n_records + 1] = every record's first byte
// in d_text (`cap` bytes of room), the total behind the last; *d_bad (4 bytes, 0 going in) = 1 if a path's allele id lies
// outside a record's map (the cell is then printed `.`)
void pgk_launch_ptpanel(const PanelDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off, uint64_t n_records,
                        char* d_text, uint64_t cap, uint32_t* d_bad, hipStream_t s);
uint32_t pgk_ptpanel_block(void);
uint32_t pgk_ptpanel_stage_bytes(void);
// pg_phase_text.hip: k_rphase over the descriptors' records
void pgk_launch_rphase(const DevContig* d_contigs, const RPhaseDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, hipStream_t s);
// ... and the packed text: d_loc [n_records], d_bsum [n_blocks], d_bbase [n_blocks + 1]: the scan's; d_off [n_records + 1] =
// every record's first byte in d_text (`cap` bytes of room), the total behind the last
void pgk_launch_ptext(const DevContig* d_contigs, const PTextDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, uint32_t* d_loc, uint32_t* d_bsum,
                      uint64_t* d_bbase, uint64_t* d_off, uint64_t n_records, char* d_text, uint64_t cap, hipStream_t s);
uint32_t pgk_ptext_block(void);
uint32_t pgk_ptext_stage_bytes(void);
// pg_record_lines.hip: d_loc [n_lines], d_bsum [n_blocks], d_bbase [n_blocks + 1]: the scan's; d_off [n_lines + 1] = every
// line's first byte in d_out (`cap` bytes of room), the total behind the last.  slotted: the kernels that read the
// descriptors' slot fields; d_contigs may be null if no descriptor reads a chain
void pgk_launch_rlines(const DevContig* d_contigs, const RLinesDesc* d_desc, uint32_t n_desc, const RLinesMember* d_members, bool slotted, uint32_t n_blocks,
                       uint32_t n_emit_blocks, uint32_t* d_loc, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off, uint64_t n_lines, char* d_out,
                       uint64_t cap, hipStream_t s);
uint32_t pgk_rlines_block(void);
uint32_t pgk_rlines_stage_bytes(void);
uint32_t pgk_rlines_lines_per_wave(uint32_t n_members, bool slotted);
// pg_record_text.hip: d_wide = uint2 {descriptor, record} of every record with more than pgk_rtext_wide_values() values;
// d_loc [n_records], d_wlen [n_wide], d_bsum [n_blocks], d_bbase [n_blocks + 1]: the scan's; d_off [n_records + 1] = every
// record's first byte in d_text (`cap` bytes of room), the total behind the last.  The two events (or null) go around
// k_rtext_emit alone.
void pgk_launch_rtext(const DevContig* d_contigs, const RTextDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                      uint32_t* d_loc, uint32_t* d_wlen, uint32_t* d_bsum, uint64_t* d_bbase, uint64_t* d_off, uint64_t n_records, char* d_text,
                      uint64_t cap, hipEvent_t emit_begin, hipEvent_t emit_end, hipStream_t s);
uint32_t pgk_rtext_block(void);
uint32_t pgk_rtext_stage_bytes(void);
uint32_t pgk_rtext_wide_values(void);
// pg_combine_records.hip: d_wide = uint2 {descriptor, record} of every record of a bubble with more than PG_AMAX alleles;
// d_stage = n_slots staging slots of `stride` 16-byte values each (max_bins quotients, then the folded map), one per block
void pgk_launch_crcalls(const DevContig* d_contigs, const CRecDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                        void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, const uint64_t* d_thr_m, const int32_t* d_thr_e, hipStream_t s);
void pgk_launch_crgl(const DevContig* d_contigs, const CRecDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                     void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, hipStream_t s);
// k_crplan_ids: *d_hit (8 bytes, all ones going in) = the lowest (group << 32 | variant) with an allele id outside the map of
// one of the variant's records
void pgk_launch_crplan_ids(const DevContig* d_contigs, const CRecDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, void* d_hit, hipStream_t s);
uint32_t pgk_combined_records_block(void);
// pg_calls.hip: the lists and staging slots of pgk_launch_rcalls, descriptors with the GL buffers
void pgk_launch_rgl(const DevContig* d_contigs, const RGlDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                    void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, hipStream_t s);
// pg_calls.hip: out[i] = the pg_gl of m[i] 2^e[i] (m normalised or 0)
void pgk_launch_gl_values(const uint64_t* d_m, const int32_t* d_e, void* d_out, uint32_t n, hipStream_t s);
// pg_calls.hip: d_wide = uint2 {descriptor, record} of every record of a bubble with more than PG_AMAX alleles; d_stage = n_slots
// staging slots of `stride` 16-byte values each (max_bins quotients, then the folded map) — one per block of k_rcalls_wide
void pgk_launch_rcalls(const DevContig* d_contigs, const RCallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                       void* d_stage, uint32_t max_bins, uint32_t stride, uint32_t n_slots, const uint64_t* d_thr_m, const int32_t* d_thr_e, hipStream_t s);
// pg_calls.hip, k_rplan_ids: the descriptors and blocks of pgk_launch_rcalls; *d_hit (8 bytes, all ones going in) = the lowest
// (chain << 32 | variant) with an allele id outside the map of one of the variant's records
void pgk_launch_rplan_ids(const DevContig* d_contigs, const RCallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, void* d_hit, hipStream_t s);
// pg_calls.hip: d_wide = uint2 {descriptor, variant} of every variant with more than PG_AMAX alleles (k_calls_wide's list)
void pgk_launch_calls(const DevContig* d_contigs, const CallsDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const void* d_wide, uint32_t n_wide,
                      const uint64_t* d_thr_m, const int32_t* d_thr_e, hipStream_t s);
uint32_t pgk_calls_block(void);
// pg_combine.hip: d_wide = uint2 {descriptor, variant} of every variant with more than PG_AMAX alleles (the wave-per-variant kernels' list)
void pgk_launch_combine(const DevContig* d_contigs, const CombineDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const uint32_t* d_members,
                        const void* d_wide, uint32_t n_wide, hipStream_t s);
void pgk_launch_ccalls(const DevContig* d_contigs, const CombineDesc* d_desc, uint32_t n_desc, uint32_t n_blocks, const uint32_t* d_members,
                       const void* d_wide, uint32_t n_wide, const uint64_t* d_thr_m, const int32_t* d_thr_e, hipStream_t s);
// k_combine_check: *d_hit (4 bytes, 0 going in) = 1 + the number of a pair whose allele_off or allele_id differ
void pgk_launch_combine_check(const DevContig* d_contigs, const CombinePair* d_pairs, uint32_t n_pairs, uint32_t max_items, uint32_t* d_hit, hipStream_t s);
uint32_t pgk_combine_block(void);
// pg_kernels.hip
void pgk_launch_prep(const DevContig* d_contigs, uint32_t n_contigs, uint32_t max_v, uint32_t max_w, uint32_t max_m4, DevTable tab, hipStream_t s);
void pgk_launch_compact(const DevContig* d_contigs, uint32_t n_contigs, hipStream_t s);
void pgk_launch_index(const DevContig* d_reps, uint32_t n_index, uint32_t max_v, uint32_t max_big, int any_split, hipStream_t s);
void pgk_launch_prep_split(const DevContig* d_contigs, uint32_t n_contigs, uint32_t max_b, uint32_t max_m4, uint32_t max_w, DevTable tab, hipStream_t s);
void pgk_launch_records(const DevContig* d_contigs, uint32_t n_contigs, uint32_t max_v, hipStream_t s);
// k_prep_bi_part / k_records_part: one part of every chain (1: the ends, 2: the middle — pg_device.h: pg_prep_middle, W = the
// band's half-width in columns); max_pv / max_pc = the most variants / columns a chain has in that part (0: no launch)
void pgk_launch_prep_part(const DevContig* d_contigs, uint32_t n_contigs, uint32_t part, uint32_t W, uint32_t max_pv, DevTable tab, hipStream_t s);
void pgk_launch_records_part(const DevContig* d_contigs, uint32_t n_contigs, uint32_t part, uint32_t W, uint32_t max_pc, hipStream_t s);
void pgk_launch_bins(const DevContig* d_contigs, uint32_t n_contigs, uint32_t max_v, uint32_t which, uint32_t max_wide, hipStream_t s);
void pgk_launch_sweep(const DevContig* d_contigs, uint32_t n_contigs, uint32_t hp_mask, int phase, hipStream_t s);
void pgk_launch_sweep_piece(const DevContig* d_contigs, uint32_t n_contigs, uint32_t piece_chunks, uint32_t piece, hipStream_t s);
void pgk_launch_sweep_chunk(const DevContig* d_contigs, uint32_t n_contigs, uint32_t hp_mask, uint32_t chunk, hipStream_t s);
void pgk_launch_sweep_small(const DevContig* d_contigs, const uint32_t* d_ids, uint32_t n_ids, int phase, uint32_t chunk, double* d_dump, hipStream_t s);
void pgk_launch_sweep_smallx(const DevContig* d_contigs, const uint32_t* d_ids, uint32_t n_ids, int phase, uint32_t chunk, double* d_dump, hipStream_t s);
uint32_t pgk_post_blocks(uint32_t n_contigs, uint32_t chunk_cols, uint32_t* cus_out);
void pgk_launch_post(const DevContig* d_contigs, uint32_t n_contigs, uint32_t chunk_cols, uint32_t chunk, hipStream_t s);
void pgk_launch_refill(const DevContig* d_contigs, uint32_t n_contigs, uint32_t chunk_cols, uint32_t chunk, int phase2, uint32_t max_blocks, hipStream_t s);
void pgk_launch_stream_handshake(uint32_t* d_words, hipStream_t s, hipStream_t s2);
void pgk_launch_phase2_persistent(const DevContig* d_contigs, uint32_t n_contigs, uint32_t post_blocks, hipStream_t s, hipStream_t s2);
void pgk_launch_emission_single(const DevContig* d_contig, DevTable tab, uint32_t v, double* out_m, int* out_e, hipStream_t s);
void pgk_launch_transition_single(double d, uint32_t H, int uniform, double* out3, hipStream_t s);
uint32_t pgk_threads_for_hp(uint32_t hp);
// pg_viterbi.hip
void pgk_launch_viterbi(const DevContig* d_contigs, uint32_t n, uint32_t max_v, uint32_t hp_bits, hipStream_t s);
}
