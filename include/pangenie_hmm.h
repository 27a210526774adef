/*
 * pangenie_hmm.h — C ABI of the MI355X-native PanGenie genotyping hot path.
 *
 * This is the drop-in boundary: everything the reference does inside
 *     HMM::HMM(...)                      (reference src/hmm.hpp:38, src/hmm.cpp:25-63)
 * for run_genotyping=true (and run_phasing=true: the Viterbi path, src/hmm.cpp:112-173, 408-511,
 * pangenie_amd/csrc/pg_viterbi.hip) — ColumnIndexer (src/columnindexer.cpp:8-33),
 * EmissionProbabilityComputer (src/emissionprobabilitycomputer.cpp:9-53),
 * TransitionProbabilityComputer (src/transitionprobabilitycomputer.cpp:8-19),
 * forward/backward columns + posterior accumulation (src/hmm.cpp:76-110, 175-405) —
 * happens behind pg_hmm_genotype_contig() / pg_job_run() on the GPU.
 *
 * Plain C: pointers + sizes, no STL, no exceptions, no torch types.  All host
 * pointers are caller-owned and only read during the call (same ownership rule
 * as the reference's borrowed unique_kmers / probabilities / only_paths
 * pointers, src/hmm.cpp:25-31).  Error convention: 0 = ok, negative = error
 * with a message in `err` (the C++ adapter rethrows std::runtime_error, which
 * is what the reference throws, e.g. src/columnindexer.cpp:18-22).
 *
 * Numeric contract: the device computes in fp64 and returns every unnormalised
 * genotype likelihood as  lik[g] * 2^lik_exp[g]  — one fp64 mantissa in [0.5,1)
 * (or 0) and one int32 exponent PER GENOTYPE BIN; the host rebuilds the
 * reference's 80-bit `long double` value with ldexpl() and does normalisation /
 * GT / GQ in long double (reference src/genotypingresult.cpp:118-210).
 * Guaranteed range: every bin holds 1e-6 relative (observed 1e-13) down to the
 * reference's own long double underflow (2^-16445), however many decades it lies
 * below its variant's largest bin, for every chain whose transitions mix
 * (recombination probability q > 0 between neighbouring columns: any gap of
 * >= 1 bp at recombrate * effective_N >= 1e-12).  The emission of a bin is
 * applied once, to the finished bin, as (mantissa, exponent); the stored columns
 * carry a bounded dynamic range (>= q^2 of their sum).  Chains WITHOUT mixing
 * (recombrate == 0 or effective_N == 0: every state evolves on its own) keep
 * 2^-1400 relative to a column's sum in fp64 where the reference keeps 2^-16445.
 */
#ifndef PANGENIE_HMM_H
#define PANGENIE_HMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK 0
#define PG_ERR_INVALID (-1)     /* bad argument / malformed batch            */
#define PG_ERR_NO_PATHS (-2)    /* "column is not covered by any paths"      */
#define PG_ERR_UNSUPPORTED (-3) /* device limits: > 1024 selected paths (> 64 with run_phasing), > 256 alleles per variant */
#define PG_ERR_DEVICE (-4)      /* HIP runtime error / no GPU                */
#define PG_ERR_NOMEM (-5)

/* ------------------------------------------------------------------ *
 *  Input: one (contig, path-subset) chain, flattened to SoA.
 *  Replaces std::vector<std::shared_ptr<UniqueKmers>>* + only_paths
 *  (reference src/uniquekmers.hpp:22-69, src/hmm.hpp:38).
 * ------------------------------------------------------------------ */
typedef struct pg_contig_batch {
    uint32_t n_variants; /* V : unique_kmers->size()                                        */
    uint32_t n_paths;    /* H : number of SELECTED paths (ColumnIndexer::nr_paths,          */
                         /*     columnindexer.cpp:23,51-53); states per column = H*H        */
    const uint64_t* variant_pos;  /* [V]   UniqueKmers::get_variant_position()              */
    const uint16_t* coverage;     /* [V]   UniqueKmers::get_coverage() (float -> u16)       */
    const uint32_t* kmer_off;     /* [V+1] prefix offsets into kmer_count                   */
    const uint16_t* kmer_count;   /* [sumK] UniqueKmers::get_readcount_of(k)                */
    const uint32_t* allele_off;   /* [V+1] prefix offsets into the allele_* arrays          */
    const uint16_t* allele_id;    /* [sumA] get_allele_ids(): ALL alleles of the object,    */
                                  /*        ascending (std::map order)                      */
    const uint8_t*  allele_flags; /* [sumA] bit0 = is_undefined_allele(a)                   */
    const uint16_t* allele_kmer_off;  /* [sumA] KmerPath::offset  (kmerpath.hpp:33)         */
    const uint32_t* allele_kmer_mask; /* [sumA] KmerPath::kmers   (16-bit masks widened):   */
                                  /* kmer k on allele a <=> 0<=k-off<32 && mask>>(k-off)&1  */
                                  /* (kmerpath.cpp:33-48)                                   */
    const uint16_t* path_allele;  /* [V*H] allele id carried by selected path p at variant  */
                                  /* v: UniqueKmers::get_allele(paths[p])                   */
} pg_contig_batch;

/* HMM constructor arguments (reference src/hmm.hpp:38, call site src/commands.cpp:160). */
typedef struct pg_hmm_params {
    long double effective_N; /* default 25000.0L; production 1e-5 (pangenie-genotype.cpp:33-45) */
    double recombrate;       /* default 1.26                                                     */
    int32_t uniform;         /* uniform transition probabilities                                 */
    int32_t run_genotyping;  /* forward-backward                                                 */
    int32_t run_phasing;     /* Viterbi path over ordered path pairs (src/hmm.cpp:112-173, 408-511): */
                             /* fills haplotype_1 / haplotype_2; at most 64 selected paths          */
    int32_t reserved;        /* call flags of the one-shot entry point: PG_CALL_ANNOUNCED; else 0                */
} pg_hmm_params;
#define PG_CALL_ANNOUNCED 1  /* this pg_hmm_genotype_contig call was announced with pg_hmm_announce(device) */

/* ------------------------------------------------------------------ *
 *  Output, caller-allocated.  Genotype bins of variant v live at
 *  lik[geno_off[v] .. geno_off[v+1]) with geno_off from
 *  pg_hmm_geno_offsets(): bin index of allele SLOTS (a<=b) of an A-allele
 *  variant is  a*A - a*(a-1)/2 + (b-a)  (lexicographic (a,b), i.e. the
 *  iteration order of the reference's std::map<pair<u16,u16>,long double>,
 *  src/genotypingresult.hpp:84).  A bin is a key of the reference's map iff
 *  kept[v] && allele_present[a] && allele_present[b] (src/hmm.cpp:368).
 * ------------------------------------------------------------------ */
typedef struct pg_contig_result {
    double*   lik;            /* [geno_off[V]] unnormalised likelihood, mantissa in [0.5,1) or 0 */
    int32_t*  lik_exp;        /* [geno_off[V]] power-of-two exponent per bin: L = lik * 2^lik_exp */
    uint8_t*  kept;           /* [V] 1 = variant is an HMM column (columnindexer.cpp:24-31)   */
    uint8_t*  allele_present; /* [sumA] 1 = allele slot occurs on a selected path             */
    uint16_t* n_kmers;        /* [V] GenotypingResult::set_unique_kmers (hmm.cpp:106-109)     */
    uint16_t* coverage;       /* [V] GenotypingResult::set_coverage                           */
    uint32_t  n_columns;      /* C = ColumnIndexer::size()                                    */
    uint32_t  reserved;
    /* run_phasing only (may be NULL): alleles of the Viterbi path's two haplotypes at kept variants  */
    /* (GenotypingResult::add_first/second_haplotype_allele, src/hmm.cpp:146-162), 0 elsewhere.  With */
    /* run_phasing the reference also sets unique_kmers / coverage of results[c] for every COLUMN     */
    /* index c < C from variant c (sic, src/hmm.cpp:164-165): n_kmers / coverage above follow that.   */
    uint16_t* haplotype_1;    /* [V] */
    uint16_t* haplotype_2;    /* [V] */
} pg_contig_result;

/* geno_off[V+1] from allele_off: geno_off[v+1]-geno_off[v] = A_v*(A_v+1)/2. */
int pg_hmm_geno_offsets(const pg_contig_batch* batch, uint64_t* geno_off);

/* ------------------------------------------------------------------ *
 *  ProbabilityTable (reference src/probabilitytable.hpp:13-29).  Built on the
 *  host in long double exactly as the reference does before the HMM runs
 *  (src/commands.cpp:846); the device receives it as (mantissa, exponent)
 *  pairs.  Out-of-range (coverage,count) pairs are evaluated on the fly
 *  (src/probabilitytable.cpp:47-53) — on the device in fp64.
 * ------------------------------------------------------------------ */
typedef struct pg_table pg_table;
pg_table* pg_table_create(uint16_t cov_min, uint16_t cov_max, uint16_t count_max,
                          long double regularization);            /* probabilitytable.cpp:28-45 */
pg_table* pg_table_create_default(void);                           /* probabilitytable.cpp:21-26 */
int  pg_table_modify(pg_table* t, uint16_t coverage, uint16_t count,
                     long double p0, long double p1, long double p2); /* :67-73, test hook */
int  pg_table_get(const pg_table* t, uint16_t coverage, uint16_t count,
                  long double out3[3]);                             /* :47-53 */
void pg_table_destroy(pg_table* t);

/* ------------------------------------------------------------------ *
 *  One-shot blocking call = the body of HMM::HMM for one (contig, subset).
 *  Thread-safe and re-entrant, the way the reference calls its constructor: N thread-pool workers at
 *  a time, one call per (contig x subset), sharing the table read-only (src/commands.cpp:949-978,
 *  :155-185).  Calls that are in flight together on one device with the same table and parameters are
 *  MERGED into one multi-chain device job by the first of them (the others sleep until their results
 *  are in their buffers); chains of a job are independent, so each caller gets exactly what it would
 *  have got alone, and an error of one caller's batch is that caller's alone (the merged job is then
 *  re-run call by call).  Environment: PG_COALESCE=0 (off), PG_COALESCE_WAIT_MS (250: the bound on waiting
 *  for an announced call); the join window (300 us), the merged jobs in flight per device (2) and the batch
 *  size (256 calls) are constants.
 *  Device arenas of finished calls are pooled for the next ones (pg_hmm_release_cache frees them).
 * ------------------------------------------------------------------ */
int pg_hmm_device_count(void);
const char* pg_hmm_version(void);
int pg_hmm_genotype_contig(const pg_contig_batch* batch, const pg_table* table,
                           const pg_hmm_params* params, int device,
                           pg_contig_result* out, char* err, size_t errlen);
/* Optional: a worker that WILL call pg_hmm_genotype_contig on `device` shortly (it is still
 * flattening its UniqueKmers) says so; a leader about to launch waits for announced calls (bounded by
 * PG_COALESCE_WAIT_MS).  The call itself then carries PG_CALL_ANNOUNCED in params->reserved; a worker
 * that gives up before calling retracts. */
void pg_hmm_announce(int device);
void pg_hmm_retract(int device);
/* {merged jobs launched, calls served, largest merge} since the process started */
int  pg_hmm_coalesce_stats(uint64_t out3[3]);

/* ------------------------------------------------------------------ *
 *  Resident job API: upload once, run many times (benchmarks, pipelines,
 *  multi-contig batches that share one launch).  All contigs of a job run
 *  concurrently (one persistent workgroup per chain direction).
 * ------------------------------------------------------------------ */
typedef struct pg_job pg_job;
/* (The six big arrays of a batch — kmer_count, allele_id, allele_flags, allele_kmer_off, allele_kmer_mask,
 * path_allele — may also be DEVICE pointers of `device`; the offset arrays, positions and coverage are read on the host.) */
pg_job* pg_job_create(int device, uint32_t n_contigs, const pg_contig_batch* batches,
                      const pg_table* table, const pg_hmm_params* params,
                      char* err, size_t errlen);
/* Runs the whole device path (prep -> forward/backward sweep -> bins) and
 * synchronises.  `stream` = hipStream_t to launch on, NULL = the job's own. */
int  pg_job_run(pg_job* job, void* stream, char* err, size_t errlen);
/* Copies contig c's results to host buffers. */
int  pg_job_fetch(pg_job* job, uint32_t contig, pg_contig_result* out, char* err, size_t errlen);
/* The same for all chains with one synchronisation: outs[n_chains], chain order. */
int  pg_job_fetch_all(pg_job* job, pg_contig_result* outs, char* err, size_t errlen);
/* Device-resident result buffers of contig c: lik f64 [n_lik], lik_exp i32 [n_lik]. */
int  pg_job_device_results(pg_job* job, uint32_t contig, void** d_lik, uint64_t* n_lik,
                           void** d_lik_exp, uint64_t* n_variants);
/* Per-kernel-class elapsed milliseconds of the LAST pg_job_run, measured with
 * hipEvents on the launch stream.  Order given by pg_job_kernel_name(). */
#define PG_N_KERNEL_CLASSES 6
int  pg_job_kernel_ms(const pg_job* job, double ms[PG_N_KERNEL_CLASSES]);
const char* pg_job_kernel_name(int cls);
/* Profiling hook: 64 in-kernel cycle counters of contig c's chain kernels, filled when the
 * library was built with -DPG_CHAIN_PROF (a measurement build; layout documented in DESIGN.md); zeros otherwise. */
int  pg_job_profile_counters(pg_job* job, uint32_t contig, uint64_t out64[64]);
/* Bytes of device memory held by the job. */
uint64_t pg_job_device_bytes(const pg_job* job);
/* How pg_job_run schedules the second half of every half-chain: 0 = fused (posterior partials formed
 * inside the sweep, one launch; chosen when many chains fill the chip), 1 = chunked (store-only sweep
 * chunks of *chunk_cols columns, posteriors of each finished chunk on the idle CUs; chosen for few
 * chains).  Override with the environment variables PG_SWEEP_MODE=fused|chunked, PG_CHUNK_COLS=n.
 * A column with more than five distinct alleles on the selected paths ("wide") is genotyped inside a fused job when its
 * chain has 16 paths (the sampled panels of production: the column costs that column); a chain of any other width with an
 * object of more than five alleles makes its job chunked, whatever is asked for.  (Round 5 refused a 16-path chain whose ONLY
 * column is wide in a fused job; since round 6 such a chain needs no sweep and is genotyped — only with PG_KERNELS=nosplit or
 * run_phasing, where the per-sample preparation of round 5 runs, pg_job_run still answers PG_ERR_UNSUPPORTED for it.) */
int  pg_job_sweep_mode(const pg_job* job, uint32_t* chunk_cols);
/* Number of chains of the job whose columns are kept as upper triangles (fused mode, H = 64, every object with at most five
 * alleles: the columns are symmetric, so phase 1 writes and phase 2 reads only the stored half — half of the
 * 16 H^2 bytes per variant of the full formulation; PG_KERNELS=notri turns it off).  For traffic accounting. */
uint32_t pg_job_triangle_chains(const pg_job* job);
/* The index pass (round 6): what the INDEX alone decides — the ColumnIndexer flags and the column list of every contig
 * (reference src/columnindexer.cpp:8-33); for the 16-path chains of fused jobs also every column's path -> local allele map,
 * transition constants (src/transitionprobabilitycomputer.cpp:8-19) and bin addresses — is formed ONCE per uploaded index,
 * inside pg_job_new / pg_cohort_new / pg_job_upload(batches != NULL), and shared by every chain (sample) over that index contig
 * (src/commands.cpp:118-138: one index, per-sample counts).  pg_job_run forms only what hangs on the sample's counts.
 * Elapsed milliseconds of the LAST index pass (hipEvents); it is NOT part of pg_job_kernel_ms. */
double pg_job_index_ms(const pg_job* job);
/* Which kernels run for which chains of this job, as text (one line per group of chains with the same plan: count, paths,
 * sweep mode, the kernels of the preparation / phase 1 / phase 2 / bins).  Writes at most `len` bytes incl. the terminator,
 * returns the length the full text needs.  For logs and DESIGN.md's table; the library takes every decision itself. */
size_t pg_job_plan(const pg_job* job, char* out, size_t len);
/* Chunked jobs with lean chains (64 paths, biallelic) that leave compute units idle: phase 1 stores every 64th column, counted
 * from the phase boundary, and k_refill_lean forms the columns between two stored ones before k_post reads them (pg_job_plan
 * names it).  The arithmetic both sides use, for tests: segment `j` (0 .. chunk_cols / 64 - 1) of `role` (0 forward, 1 backward)
 * that chunk `chunk` of phase 2 reads — returns 1 and out = {column it resumes from, first, last column it stores}, 0 when the
 * chain of n_columns has no such segment, -1 for arguments outside the scheme (chunk_cols no multiple of 64).
 * pg_sparse_stored_by_chain: 1 if the chain itself stores `column` (its role's phase-1 half is column < n_columns / 2 for role 0). */
int pg_sparse_segment(uint32_t n_columns, uint32_t chunk_cols, uint32_t chunk, uint32_t role, uint32_t j, uint32_t out[3]);
int pg_sparse_stored_by_chain(uint32_t n_columns, uint32_t role, uint32_t column);
/* Where every chain with columns is such a chain, the chunk sweeps of phase 2 store every 64th column too (the checkpoints go on
 * from the phase boundary, into an area of the chain's own), and a second k_refill_lean per chunk forms the chunk's columns behind
 * its sweep.  Segment `j` of chunk `chunk` itself: returns 1 and out = {column it resumes from, lowest, highest column it stores —
 * the highest (forward role) or lowest (backward role) is the next checkpoint, except at the end of the half}, 0 / -1 as above.
 * pg_sparse_chunk_stored_by_chain: 1 if the chain itself stores `column` of its role's phase-2 half. */
int pg_sparse_chunk_segment(uint32_t n_columns, uint32_t chunk_cols, uint32_t chunk, uint32_t role, uint32_t j, uint32_t out[3]);
int pg_sparse_chunk_stored_by_chain(uint32_t n_columns, uint32_t role, uint32_t column);
/* Such a job runs phase 1 as one launch per piece: the phase-1 columns of a role whose partner chunk of phase 2 lies in
 * [piece * piece_chunks, (piece + 1) * piece_chunks), the farthest piece first; the partner columns of a piece's chunks are refilled
 * beside the pieces behind it (pg_job_plan names the number of pieces; PG_PIECE_CHUNKS sets piece_chunks).  Returns 1 and
 * out = {lowest, highest column of the piece}, 0 when the role has no column that far from the phase boundary, -1 as above. */
int pg_sparse_piece_range(uint32_t n_columns, uint32_t chunk_cols, uint32_t piece_chunks, uint32_t piece, uint32_t role, uint32_t out[2]);
/* The column records of such a launch reach the kernel in blocks of 64, two of them in a ring; the launch numbers its steps so
 * that its groups of 64 steps (63 store-free, one storing) begin at a multiple of 64, and a group parks and expands the next
 * block at two fixed steps.  The numbering of a launch, for tests: form 0 = phase 1 in one launch, 1 = piece `arg` of phase 1,
 * 2 = chunk sweep `arg` of phase 2.  Returns 1 and out = {column of the first step, number of steps, steps in front of the first
 * group, number of the first step, step of a group that parks a block, step of a group that expands it}; 0: the launch has no
 * step; -1 as above. */
int pg_lean_ring_schedule(uint32_t n_columns, uint32_t chunk_cols, uint32_t piece_chunks, uint32_t role, uint32_t form, uint32_t arg, uint32_t out[6]);
/* Byte offset, inside the ring, of the 256-byte image that holds everything a step reads of record number `record`. */
uint32_t pg_lean_ring_image_offset(uint32_t record);
/* A job in pieces whose chains are all-biallelic prepares only the ENDS of its chains ahead of phase 1 — what the first `early`
 * pieces read — and their MIDDLE on the second stream beside those pieces (pg_job_plan says which schedule a job takes;
 * PG_PREP_EARLY_PIECES sets `early`, PG_KERNELS=prepahead keeps the whole preparation ahead).  The middle of a chain of n_columns
 * when the job has n_pieces pieces: returns 1 and out_cols = {first column of the middle, first column behind it}; with
 * col_variant (the n_columns ascending variant ids of the columns) also out_vars = the same for its n_variants variants — a
 * variant goes with its column, one that is no column with the next column below it.  0: n_pieces < early + 1 (the preparation
 * stays ahead), -1 as above.  Either output may be NULL. */
int pg_prep_parts(uint32_t n_columns, uint32_t chunk_cols, uint32_t piece_chunks, uint32_t n_pieces, uint32_t early,
                  const uint32_t* col_variant, uint32_t n_variants, uint32_t out_cols[2], uint32_t out_vars[2]);
/* Item `u` of part 1 (the ends: what lies below the middle, then what lies above it) or part 2 (the middle) of n columns or
 * variants whose middle is [lo, hi) — how the kernels of a part map their threads onto it; n: the part has no item u. */
uint32_t pg_prep_part_member(uint32_t part, uint32_t lo, uint32_t hi, uint32_t n, uint32_t u);
/* Elapsed milliseconds of the Viterbi kernels (run_phasing) of the LAST pg_job_run, hipEvents on the launch stream. */
double pg_job_viterbi_ms(const pg_job* job);
void pg_job_destroy(pg_job* job);

/* The inputs a job holds on the device: sizes of chain `contig`'s panel, and the arrays themselves back on the host
 * (caller-allocated by those sizes; any pointer may be NULL).  For jobs whose panel was formed on the device
 * (include/pangenie_sampler.h: pg_sampler_then_job) this is the only way to see it. */
int  pg_job_panel_sizes(const pg_job* job, uint32_t contig, uint32_t* n_variants, uint32_t* n_paths,
                        uint64_t* sum_kmers, uint64_t* sum_alleles);
int  pg_job_fetch_panel(pg_job* job, uint32_t contig, uint32_t* kmer_off, uint16_t* kmer_count,
                        uint32_t* allele_off, uint16_t* allele_id, uint8_t* allele_flags,
                        uint16_t* allele_kmer_off, uint32_t* allele_kmer_mask, uint16_t* path_allele,
                        char* err, size_t errlen);

/* pg_job_create with an error code instead of a NULL: PG_ERR_INVALID (malformed batch),
 * PG_ERR_UNSUPPORTED (limits above), PG_ERR_NOMEM (device allocation), PG_ERR_DEVICE. */
int  pg_job_new(int device, uint32_t n_contigs, const pg_contig_batch* batches,
                const pg_table* table, const pg_hmm_params* params,
                pg_job** out, char* err, size_t errlen);
/* Number of chains of a job (= n_contigs, or n_samples * n_contigs for a cohort job): the range of
 * the `contig` argument of pg_job_fetch / pg_job_device_results / pg_job_profile_counters. */
uint32_t pg_job_n_chains(const pg_job* job);

/* ------------------------------------------------------------------ *
 *  Cohort jobs: many samples against ONE index.
 *  The index (`*_UniqueKmersMap.cereal`: positions, alleles, k-mer masks, path -> allele) is
 *  shared by all samples; only the read k-mer counts and the local coverage differ per
 *  sample (reference src/commands.cpp:118-138, README.md:128).  The index arrays are
 *  uploaded once; every (sample, contig) pair is an independent chain of the job:
 *      chain id = sample * n_contigs + contig.
 *  `index[c].kmer_count` / `.coverage` are ignored (may be NULL).
 * ------------------------------------------------------------------ */
typedef struct pg_sample_counts {
    const uint16_t* const* kmer_count; /* [n_contigs] -> [sumK of contig c]  UniqueKmers::update_readcount */
    const uint16_t* const* coverage;   /* [n_contigs] -> [V of contig c]     UniqueKmers::set_coverage     */
} pg_sample_counts;
int  pg_cohort_new(int device, uint32_t n_contigs, const pg_contig_batch* index,
                   uint32_t n_samples, const pg_sample_counts* samples,
                   const pg_table* table, const pg_hmm_params* params,
                   pg_job** out, char* err, size_t errlen);

/* Re-uploads the inputs of a resident job (same shapes as at creation): what a pipeline does
 * with the next set of read counts.  `samples` = NULL for a job made by pg_job_create/new (the
 * batches carry their own counts), else the cohort's per-sample arrays (`batches` may then be
 * NULL to keep the resident index and upload the counts only). */
int  pg_job_upload(pg_job* job, const pg_contig_batch* batches, const pg_sample_counts* samples,
                   char* err, size_t errlen);
/* pg_job_upload followed by pg_job_run (on the job's own stream) in ONE call — the arrays stay valid until it returns, so a job of a
 * few long chains (a whole genome's chromosomes) uploads the inputs of its longest chains first, starts their preparation and phase 1
 * and lets the other chains' inputs cross PCIe meanwhile (round 6; the one-shot pg_hmm_genotype_contig does the same inside).  Same
 * results as the two calls, bit for bit.  pg_job_host_seconds: [1] then counts only what the caller waited for in front of the run. */
int  pg_job_upload_run(pg_job* job, const pg_contig_batch* batches, const pg_sample_counts* samples, char* err, size_t errlen);
/* The same for a cohort job WITHOUT stalling the device: pg_job_upload_begin starts copying the next batch of samples
 * (reference: one PanGenie run per sample re-reads its counts, src/commands.cpp:118-138) into the job's second set of
 * per-sample arrays — host threads pack the counts into a pinned staging buffer, a few large H2D copies on a copy stream of
 * the job's own — and returns at once; pg_job_run keeps genotyping the current batch meanwhile.  pg_job_upload_end waits
 * for the copy and makes the new batch the one the next pg_job_run reads.  Call order of a pipeline:
 *     upload_begin(n+1); run(n); fetch(n); upload_end(n+1); upload_begin(n+2); run(n+1); ...
 * The arrays behind `samples` must stay valid and unchanged until pg_job_upload_end returns; results of the previous run
 * must be fetched BEFORE pg_job_upload_end (it invalidates them: fetch then returns PG_ERR_INVALID until the next run). */
int  pg_job_upload_begin(pg_job* job, const pg_sample_counts* samples, char* err, size_t errlen);
int  pg_job_upload_end(pg_job* job, char* err, size_t errlen);
/* Host wall seconds: [0] device allocation at creation, [1] last input upload (H2D; after pg_job_upload_end: what it waited),
 * [2] last pg_job_run, [3] last pg_job_fetch_all / sum of pg_job_fetch since the last run. */
int  pg_job_host_seconds(const pg_job* job, double out4[4]);
/* Input bytes moved H2D by the last upload: [0] index arrays, [1] per-sample arrays. */
int  pg_job_upload_bytes(const pg_job* job, uint64_t out2[2]);
/* All chains' posteriors as two packed device ranges, chain after chain (what a multi-GPU
 * gather sends): lik f64 [n_lik_total], lik_exp i32 [n_lik_total]. */
int  pg_job_packed_results(pg_job* job, void** d_lik, void** d_lik_exp, uint64_t* n_lik_total);
/* The one-shot call keeps the device arenas of its finished jobs in a pool for the next calls
 * (per device at most PG_ARENA_POOL_GB, default 70 % of the device's memory); this releases them. */
void pg_hmm_release_cache(void);

/* ------------------------------------------------------------------ *
 *  Multi-GPU: contigs (x subsets x samples) shard across the GPUs of a node with no data-path
 *  collective — the reference already runs them as independent jobs and only merges results
 *  (src/commands.cpp:955-978, 163-177).  The ONE exchange is the collection of every rank's
 *  packed posteriors on the root: grouped RCCL point-to-point sends over xGMI, each block exactly
 *  as long as that rank's data (lik f64 + lik_exp i32 per genotype bin).  RCCL is loaded at run
 *  time, only when a communicator is made.
 * ------------------------------------------------------------------ */
typedef struct pg_comm pg_comm;
/* process-per-GPU: rank 0 makes the id, the host hands it to the other ranks (file, MPI, ...) */
int  pg_comm_unique_id(uint8_t id128[128], char* err, size_t errlen);
int  pg_comm_init(const uint8_t id128[128], int world, int rank, int device,
                  pg_comm** out, char* err, size_t errlen);
/* one process, several GPUs: out_comms[i] = rank i on devices[i] */
int  pg_comm_init_all(int n_devices, const int* devices, pg_comm** out_comms, char* err, size_t errlen);
int  pg_comm_rank(const pg_comm* comm);
int  pg_comm_world(const pg_comm* comm);
void pg_comm_destroy(pg_comm* comm);
/* Every rank calls this once per run with its job (NULL on a rank without chains) and the plan
 * n_lik_per_rank[world] (genotype bins each rank holds; known to every host up front).  On `root`,
 * d_lik_all (f64) / d_exp_all (i32) are device buffers of sum(n_lik_per_rank) elements: rank r's
 * block lands at offset sum_{q<r} n_lik_per_rank[q], in that rank's chain order.  Blocking. */
int  pg_hmm_gather(pg_comm* comm, pg_job* job, int root, const uint64_t* n_lik_per_rank,
                   void* d_lik_all, void* d_exp_all, char* err, size_t errlen);
/* the same for the n_local communicators one process holds (pg_comm_init_all) */
int  pg_hmm_gather_all(int n_local, pg_comm* const* comms, pg_job* const* jobs, int root,
                       const uint64_t* n_lik_per_rank, void* d_lik_all, void* d_exp_all,
                       char* err, size_t errlen);
/* the same into HOST buffers of the root's process (temporary device buffers inside) */
int  pg_hmm_gather_to_host(int n_local, pg_comm* const* comms, pg_job* const* jobs, int root,
                           const uint64_t* n_lik_per_rank, double* h_lik_all, int32_t* h_exp_all,
                           char* err, size_t errlen);

/* ------------------------------------------------------------------ *
 *  Unit-level entry points (device), mirroring the reference classes the
 *  reference's own unit tests exercise.
 * ------------------------------------------------------------------ */
/* EmissionProbabilityComputer (emissionprobabilitycomputer.cpp:9-34): A x A table over ALL
 * allele slots of variant `v` (row-major, slot order), after the all_zeros rule. */
int pg_emission_table(const pg_contig_batch* batch, const pg_table* table, uint32_t v,
                      int device, long double* out_AxA, int32_t* all_zeros,
                      char* err, size_t errlen);
/* TransitionProbabilityComputer (transitionprobabilitycomputer.cpp:8-19):
 * out3 = {no switch, one switch, two switches}. */
int pg_transition_probs(uint64_t from_pos, uint64_t to_pos, double recombrate,
                        uint32_t nr_paths, int uniform, long double effective_N,
                        int device, double out3[3], char* err, size_t errlen);

/* ------------------------------------------------------------------ *
 *  Genotype calls formed on the device: GT and GQ per variant, 8 bytes each, instead of 12 bytes per
 *  genotype bin (pangenie_amd/csrc/pg_calls.hip).  What the host does per variant in
 *  long double — GenotypingResult::normalize, get_likeliest_genotype, get_genotype_quality (reference
 *  src/genotypingresult.cpp:118-210) on the keys of the variant's map — is done in integer arithmetic
 *  that gives the long double's bits; the records hold the same GT and GQ.  The bins stay where they
 *  are: pg_job_fetch* are not affected.
 * ------------------------------------------------------------------ */
#ifndef PG_CALL_DEFINED /* (the same in pangenie_amd/csrc/pg_calls.h) */
#define PG_CALL_DEFINED
typedef struct pg_call {
    uint16_t allele_1, allele_2; /* allele IDS (not slots) of the likeliest genotype, allele_1 <= allele_2; */
                                 /* 0xFFFF / 0xFFFF unless flags == PG_CALL_OK                              */
    uint16_t gq;                 /* get_genotype_quality: 0 .. 192, or 10000                               */
    uint16_t flags;
} pg_call;
#endif
#define PG_CALL_OK 0         /* a unique likeliest genotype                                                      */
#define PG_CALL_NONE 1       /* ./. : not a kept column, no key, or every bin zero                               */
#define PG_CALL_NOT_UNIQUE 2 /* ./. : another genotype within 1e-10 of the best (genotypingresult.cpp:164-172)   */
#define PG_CALL_DEFERRED 3   /* not decided on the device: the variant's largest bin lies below 2^-16300, next to */
                             /* long double's subnormals; form the call on the host from this variant's bins      */
/* Forms the calls of every chain of a job that has run (one launch per kernel, on the job's stream; blocking).
 * The record buffer (8 bytes x the variants of all chains) is allocated by the first call, outside the job's
 * arena, and freed by pg_job_destroy.  PG_ERR_INVALID before pg_job_run, after pg_job_upload_end or a count
 * plan's fill invalidated the run, and for a job without run_genotyping. */
int  pg_job_calls(pg_job* job, char* err, size_t errlen);
/* Chain `chain`'s records, out[V] (after pg_job_calls). */
int  pg_job_fetch_calls(pg_job* job, uint32_t chain, pg_call* out, char* err, size_t errlen);
/* The same for all chains, outs[n_chains] (a chain without variants may have NULL): copies queued on the job's
 * stream, one synchronisation. */
int  pg_job_fetch_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen);
/* Device-resident records of chain `chain`: pg_call [n]. */
int  pg_job_device_calls(pg_job* job, uint32_t chain, void** d_calls, uint64_t* n);
/* Elapsed milliseconds of the kernels of the LAST pg_job_calls (hipEvents on the job's stream). */
double pg_job_calls_ms(const pg_job* job);
/* Unit entry point: the calls of n_variants variants from host arrays laid out as pg_contig_batch /
 * pg_contig_result lay them out (allele_off [V+1], allele_id / allele_present [sumA], kept [V], lik / lik_exp
 * [sum A (A + 1) / 2]), through the same kernels; out[V].  PG_ERR_DEVICE without a device. */
int  pg_calls_from_bins(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id,
                        const uint8_t* kept, const uint8_t* allele_present, const double* lik,
                        const int32_t* lik_exp, pg_call* out);

/* ------------------------------------------------------------------ *
 *  Genotype calls per VCF RECORD (DESIGN.md 4e "Records").  The index builder merges records closer than
 *  k - 1 into one bubble; Graph::write_genotypes takes the bubble apart again: the bubble's normalised
 *  likelihoods are folded onto each record's own alleles (Variant::separate_variants, reference
 *  src/variant.cpp:357-384), genotypes over alleles of undefined sequence are dropped and the rest
 *  renormalised (get_specific_likelihoods), then likeliest genotype and quality (src/graph.cpp:217-273).
 *  The same on the device, in the integer arithmetic of pg_job_calls: one pg_call per record, holding the
 *  GT and GQ columns of the VCF.  What a bubble means for its records depends on the index alone: the
 *  RECORD PLAN of an index contig, uploaded once and shared by every chain (sample) over that contig.
 *  Limits as for pg_job_calls (PG_CALL_DEFERRED: every record of such a bubble); a record has at most 256
 *  alleles (PG_ERR_UNSUPPORTED).  `ignore_imputed` is the caller's (a bubble's k-mer count is in kmer_off).
 * ------------------------------------------------------------------ */
typedef struct pg_record_plan {
    uint32_t n_variants;        /* V: the index contig's bubbles                                                      */
    uint32_t n_records;         /* R = rec_off[V]                                                                     */
    const uint32_t* rec_off;    /* [V+1] bubble v owns the records rec_off[v] .. rec_off[v+1] - 1, at least one       */
    const uint32_t* map_off;    /* [R+1]                                                                              */
    const uint16_t* map;        /* map[map_off[r] + id] = the record allele that bubble allele ID `id` carries        */
                                /* (allele_combinations[id][r]); by id, not by slot, for id < map_off[r+1]-map_off[r] */
    const uint16_t* n_alleles;  /* [R] alleles of the record (reference allele included)                              */
    const uint32_t* vcf_off;    /* [R+1] vcf_off[r+1] - vcf_off[r] == n_alleles[r]                                    */
    const uint16_t* vcf_index;  /* per record allele: its index among the record's DEFINED alleles (the GT number),   */
                                /* 0xFFFF if its sequence is undefined; allele 0 is always defined                    */
} pg_record_plan;
#define PG_CALL_EMPTY 0x100  /* with PG_CALL_OK: 0/0, GQ 10000 because the bubble has no likelihoods at all (not a   */
                             /* kept column, no allele on a selected path), as the VCF prints it, not from evidence  */
/* Checks and uploads the plan of index contig `index_contig` (0 .. n_contigs - 1 of pg_job_create / pg_cohort_new); a
 * second plan for the same contig replaces the first.  Device memory outside the arena, freed by pg_job_destroy.
 * PG_ERR_INVALID: n_variants is not the contig's, offsets that do not start at 0 or do not grow (a bubble without a
 * record), vcf_off that does not follow n_alleles, a map entry >= the record's n_alleles, a vcf_index that is not the
 * running count of defined alleles.  PG_ERR_UNSUPPORTED: a record with more than 256 alleles. */
int  pg_job_record_plan(pg_job* job, uint32_t index_contig, const pg_record_plan* plan, char* err, size_t errlen);
/* One plan for every index contig ix with ix % n_contigs == contig: the chains sample * n_contigs + contig of a sampled
 * cohort job (pg_sampler_cohort_new[_device]: every chain is its own index contig).  Checked once, uploaded once and
 * referred to by all members; a later pg_job_record_plan on one member replaces that member's reference
 * alone, a later strided call those of all its members; the device copy is freed with its last reference and by
 * pg_job_destroy.  PG_ERR_INVALID: n_contigs == 0, contig >= n_contigs, a number of index contigs that is no multiple of
 * n_contigs, a member whose n_variants is not the plan's; the plan's own refusals as above.  Nothing is attached then. */
int  pg_job_record_plan_strided(pg_job* job, uint32_t contig, uint32_t n_contigs, const pg_record_plan* plan, char* err, size_t errlen);
/* Forms one pg_call per record for every chain whose index contig has a plan (a chain without one is left out), on the
 * job's stream; blocking.  allele_1 <= allele_2 are GT numbers: indices among the record's defined alleles.  Refusals
 * as pg_job_calls; PG_ERR_INVALID also if an allele id of a chain lies outside a record's map (checked here, on the
 * device, whenever a plan or the index has changed: a sampled panel's ids exist only there, after its job was made; the
 * message names the lowest chain and its lowest variant). */
int  pg_job_record_calls(pg_job* job, char* err, size_t errlen);
/* Chain `chain`'s records, out[R of its index contig's plan] (after pg_job_record_calls); nothing for a chain without a plan. */
int  pg_job_fetch_record_calls(pg_job* job, uint32_t chain, pg_call* out, char* err, size_t errlen);
/* The same for all chains, outs[n_chains] (NULL allowed where a chain has no records): one synchronisation. */
int  pg_job_fetch_record_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen);
/* Device-resident records of chain `chain`: pg_call [n] (n = 0 for a chain without a plan). */
int  pg_job_device_record_calls(pg_job* job, uint32_t chain, void** d_calls, uint64_t* n);
/* Elapsed milliseconds of the kernels of the LAST pg_job_record_calls. */
double pg_job_record_calls_ms(const pg_job* job);
/* Unit entry point: the record calls of n_variants bubbles from host arrays (as pg_calls_from_bins) and a plan, through
 * the same kernels; out[plan->n_records].  The plan is checked first (PG_ERR_INVALID / PG_ERR_UNSUPPORTED as above, the
 * allele ids included); then PG_ERR_DEVICE without a device: there is no host fallback. */
int  pg_record_calls_from_bins(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id,
                               const uint8_t* kept, const uint8_t* allele_present, const double* lik,
                               const int32_t* lik_exp, const pg_record_plan* plan, pg_call* out);

/* ------------------------------------------------------------------ *
 *  The GL column per VCF RECORD: log10 of the likelihood of every genotype over the record's
 *  defined alleles, as Graph::write_genotypes prints it (reference src/graph.cpp:243-274) — after the fold onto
 *  the record's alleles and get_specific_likelihoods, `setprecision(4) << log10(likelihood)`.  A value is what the
 *  text shows: the four significant decimal digits of log10l(L).  The likelihood is formed in the integer
 *  arithmetic of pg_job_record_calls; the logarithm is fp64 with a stated error bound, and a value whose fourth
 *  digit that error could change is PG_GL_DEFERRED (about 2e-9 of all values).  With pg_job_record_calls, no bin
 *  has to leave the device to write a sample's VCF lines.
 * ------------------------------------------------------------------ */
#ifndef PG_GL_DEFINED /* (the same in pangenie_amd/csrc/pg_calls.h) */
#define PG_GL_DEFINED
typedef struct pg_gl { int16_t mant; int16_t exp10; } pg_gl;
/* mant in +-[1000, 9999]: log10(L) = mant * 10^(exp10 - 3), the four digits "%.4Lg" prints; the sign of mant is the log's */
/* mant == 0 && exp10 == 0 : L == 1 exactly, prints "0"                                                                 */
#define PG_GL_NEG_INF  (-32768) /* in exp10 (mant 0): L == 0 or no such key, prints "-inf"                               */
#define PG_GL_DEFERRED (-32767) /* in exp10 (mant 0): not decided on the device, form it on the host from the bins       */
#endif
/* gl_off[R + 1]: record r with nd defined alleles owns the nd (nd + 1) / 2 values gl_off[r] .. gl_off[r + 1] - 1 of a
 * chain, genotype (a <= b) over defined-allele indices at b (b + 1) / 2 + a (the VCF's order).  Host only; the offsets
 * depend on the plan alone.  PG_ERR_INVALID / PG_ERR_UNSUPPORTED: null arguments, or a plan pg_job_record_plan refuses. */
int  pg_record_gl_offsets(const pg_record_plan* plan, uint64_t* gl_off);
/* Forms the GL values of every chain whose index contig has a plan (a chain without one is left out), on the job's
 * stream; blocking.  The buffer (4 bytes x the values of all chains) is allocated by the first call, outside the
 * arena, and freed by pg_job_destroy (PG_ERR_NOMEM if it does not fit).  Refusals as pg_job_record_calls.  Every
 * value of a bubble whose largest bin lies below 2^-16300 is PG_GL_DEFERRED, as is a nonzero likelihood below it. */
int  pg_job_record_gl(pg_job* job, char* err, size_t errlen);
/* Chain `chain`'s values, out[gl_off[R]] (after pg_job_record_gl); nothing for a chain without a plan. */
int  pg_job_fetch_record_gl(pg_job* job, uint32_t chain, pg_gl* out, char* err, size_t errlen);
/* The same for all chains, outs[n_chains] (NULL allowed where a chain has no values): one synchronisation. */
int  pg_job_fetch_record_gl_all(pg_job* job, pg_gl* const* outs, char* err, size_t errlen);
/* Device-resident values of chain `chain`: pg_gl [n] (n = 0 for a chain without a plan). */
int  pg_job_device_record_gl(pg_job* job, uint32_t chain, void** d_gl, uint64_t* n);
/* Elapsed milliseconds of the kernels of the LAST pg_job_record_gl. */
double pg_job_record_gl_ms(const pg_job* job);
/* The packed fetches.  The records and the GL values lie chain after chain on the device:
 * calls_first[n_chains + 1] / gl_first[n_chains + 1] (either may be NULL) give every chain's offset, in elements, in the
 * two buffers (no padding between chains: chain c owns [first[c], first[c + 1])).  calls_first after pg_job_record_calls,
 * gl_first after pg_job_record_gl: PG_ERR_INVALID otherwise, and when both are NULL. */
int  pg_job_record_first(pg_job* job, uint64_t* calls_first, uint64_t* gl_first, char* err, size_t errlen);
/* All records / all GL values of all chains, out[n] with n = calls_first[n_chains] / gl_first[n_chains]: ONE copy on the
 * job's stream and one synchronisation.  PG_ERR_INVALID as the per-chain fetches, and when n is not the buffer's length. */
int  pg_job_fetch_record_calls_packed(pg_job* job, pg_call* out, uint64_t n, char* err, size_t errlen);
int  pg_job_fetch_record_gl_packed(pg_job* job, pg_gl* out, uint64_t n, char* err, size_t errlen);
/* Unit entry point: the GL values of the plan's records from host arrays (as pg_record_calls_from_bins), through the
 * same kernels; out[gl_off[R]].  The plan is checked first; then PG_ERR_DEVICE without a device: no host fallback. */
int  pg_record_gl_from_bins(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id,
                            const uint8_t* kept, const uint8_t* allele_present, const double* lik,
                            const int32_t* lik_exp, const pg_record_plan* plan, pg_gl* out);
/* Unit entry point of the digits alone: out[i] = the GL of the likelihood m[i] * 2^e[i] (m[i] in [2^63, 2^64), or 0
 * with e[i] == 0: PG_ERR_INVALID otherwise), by the device's own log10 / log1p.  PG_ERR_DEVICE without a device. */
int  pg_gl_from_values(int device, uint64_t n, const uint64_t* m, const int32_t* e, pg_gl* out);
/* Host only: the text `ostream << setprecision(4)` gives of the value ("%.4g" of the decimal; "-inf"; "0"), its
 * length; -1 for PG_GL_DEFERRED, an encoding that is none of the above, or a buffer too small (32 bytes suffice). */
int  pg_gl_text(pg_gl value, char* buf, size_t len);

/* ------------------------------------------------------------------ *
 *  The sample column as TEXT: the bytes of `GT:GQ:GL:KC` of every VCF record, formed on the device
 *  from the record calls, the record GLs and the chain's coverage, so that writing a sample's VCF is a splice of these
 *  bytes behind the fixed columns.  The text of a record has no terminator and no separator:
 *    `a1/a2:gq:` if (flags & 0xFF) == PG_CALL_OK and the record is not a no-call (PG_CALL_EMPTY prints 0/0:10000:),
 *    else `.:.:`; the GL values as pg_gl_text prints them, joined by `,`; `:` and KC in decimal.
 *  A record is left to the HOST — length 0, no bytes — if its call is PG_CALL_DEFERRED, if one of its values is
 *  PG_GL_DEFERRED (or one pg_gl_text refuses), or if it has fewer than 3 values.  The text of all records is packed:
 *  chain after chain, record after record, no gaps.  Not covered: the records of combined groups.  (The phasing column
 *  GT:KC is a text family of its own: 4e-9, below.)
 *  The splice itself — whole lines, every sample's column behind the fixed ones — is the next section's (4e-7).
 * ------------------------------------------------------------------ */
/* 19 n_records + 11 n_gl_total: bytes that always suffice (255/255:10000: is 14, a value at most 10, a comma between
 * values, :65535 is 6).  Host only. */
uint64_t pg_record_text_bound(uint64_t n_records, uint64_t n_gl_total);
/* Forms the text of every chain whose index contig has a plan (a chain without one is left out), on the job's stream;
 * blocking.  Forms the record calls and the record GLs first where they are not formed for this run.  KC and UK (the
 * bubble's k-mers) follow pg_job_fetch: both 0 for a chain without a kept column; KC is read from the chain's coverage
 * on the device.  A record is a no-call if ignore_imputed and UK == 0.  Refusals as pg_job_record_calls.  The buffer
 * (pg_record_text_bound of all records and values, and 12 bytes per record) lies outside the arena and is freed by
 * pg_job_destroy.  A later run, a new plan or index make the text stale: the fetches answer PG_ERR_INVALID until it is
 * formed again; forming it with another ignore_imputed replaces it. */
int  pg_job_record_text(pg_job* job, int ignore_imputed, char* err, size_t errlen);
/* text_first[n_chains + 1]: every chain's first byte in the packed text; text_first[n_chains] = its length. */
int  pg_job_record_text_first(pg_job* job, uint64_t* text_first, char* err, size_t errlen);
/* Chain `chain`'s bytes, text[n_bytes] with n_bytes = text_first[chain + 1] - text_first[chain] (PG_ERR_INVALID
 * otherwise), and, unless NULL, off[R + 1]: record r's text is text[off[r] .. off[r + 1]), relative to the chain's
 * first byte; records in the order of pg_job_fetch_record_calls. */
int  pg_job_fetch_record_text(pg_job* job, uint32_t chain, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
/* All chains: text[n_bytes], n_bytes = text_first[n_chains], ONE copy; off[R_total + 1] (or NULL) absolute in it,
 * records in the order of pg_job_record_first's calls_first. */
int  pg_job_fetch_record_text_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
/* Device-resident text of chain `chain`: *d_text = its first byte, *d_off = uint64 [n_records + 1] offsets that are
 * ABSOLUTE in the packed text (d_off[0] is the chain's first byte there). */
int  pg_job_device_record_text(pg_job* job, uint32_t chain, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes);
/* Elapsed milliseconds of the kernels of the LAST pg_job_record_text (lengths, scan, text), and of the kernel that
 * writes the narrow records' text alone. */
double pg_job_record_text_ms(const pg_job* job);
double pg_job_record_text_emit_ms(const pg_job* job);
/* Unit entry point: the text of n_records records from host arrays, through the same kernels: calls[R], record r's
 * values gl[gl_off[r] .. gl_off[r + 1]), kc[R], no_call[R] (or NULL: none); off[R + 1] and text[cap] come back.
 * PG_ERR_INVALID, before any device is asked for: null arrays, gl_off that does not start at 0 or shrinks,
 * cap < pg_record_text_bound(R, gl_off[R]), a PG_CALL_OK call with a GT number above 255 or a GQ above 10000 (the bound
 * counts on them).  Then PG_ERR_DEVICE without a device: no host fallback. */
int  pg_record_text_from_fields(int device, uint64_t n_records, const pg_call* calls, const uint64_t* gl_off, const pg_gl* gl,
                                const uint16_t* kc, const uint8_t* no_call, uint64_t* off, char* text, uint64_t cap);

/* ------------------------------------------------------------------ *
 *  Record LINES: whole VCF lines of a cohort joined on the device.  The MEMBERS of index contig k are
 *  the chains over k in ascending chain id (pg_cohort_new: samples 0 .. S-1; a job whose chains have index contigs of
 *  their own: that one chain).  With a record plan of R records and a PREFIX — R byte strings, packed, prefix_off[R + 1],
 *  the caller's: CHROM .. FORMAT without a trailing tab — the line of record r is
 *      prefix[r]  ('\t' text_s[r]) for every member s in order  '\n'
 *  with text_s[r] the bytes pg_job_record_text formed.  A line is the HOST's — length 0, nothing written — if any
 *  member's text of the record has length 0.  Lines are packed: record after record, index contig after index contig,
 *  no gaps.  Prefix and texts are opaque bytes of any length, 0 included.  Limits: the lines of 256 consecutive records
 *  stay below 4 GiB.  Not covered: the combined (-a) record families.  (The lines of the phasing column: 4e-9, below.)
 * ------------------------------------------------------------------ */
/* prefix_bytes + text_bytes + n_records (n_members + 1): reached exactly when no line is the host's.  Host only. */
uint64_t pg_record_lines_bound(uint64_t n_records, uint64_t n_members, uint64_t prefix_bytes, uint64_t text_bytes);
/* Uploads the prefix of one index contig: off[R + 1] with R the records of its plan, bytes[off[R]]; a second call
 * replaces it, a new record plan or a new index for that contig drops it.  PG_ERR_INVALID: a null job or null arrays
 * (bytes may be NULL only if off[R] == 0), index_contig out of range, no record plan on it, off[0] != 0 or off shrinks. */
int  pg_job_line_prefix(pg_job* job, uint32_t index_contig, const uint64_t* off, const char* bytes, char* err, size_t errlen);
/* Forms the lines of every index contig that has a plan, a prefix and at least one member (the others are left out: no
 * error), on the job's stream; blocking.  PG_ERR_INVALID unless pg_job_record_text has been called for this run and
 * these plans: it does not form the text itself (ignore_imputed is the text's argument).  The buffer — the exact bound,
 * and 8 bytes a line and the scan's words — lies outside the arena, is made by the first call and freed by
 * pg_job_destroy; PG_ERR_NOMEM if it does not fit.  The lines are stale exactly when the text they were joined from is
 * stale or formed again, or a prefix changed: the fetches then answer PG_ERR_INVALID. */
int  pg_job_record_lines(pg_job* job, char* err, size_t errlen);
/* *n_index_contigs (or NULL) = the job's index contigs; line_first / byte_first (each [n_index_contigs + 1], or NULL):
 * every index contig's first line / first byte in the packed lines.  With both arrays NULL only the number is reported
 * (for any job); otherwise the lines must be formed and current. */
int  pg_job_record_lines_first(pg_job* job, uint64_t* n_index_contigs, uint64_t* line_first, uint64_t* byte_first, char* err, size_t errlen);
/* One index contig's bytes, text[n_bytes] with n_bytes = byte_first[k + 1] - byte_first[k] (PG_ERR_INVALID otherwise),
 * and, unless NULL, off[R + 1] relative to the contig's first byte. */
int  pg_job_fetch_record_lines(pg_job* job, uint32_t index_contig, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
/* All index contigs: text[n_bytes], n_bytes = byte_first[n_index_contigs], ONE copy; off[n_lines + 1] (or NULL) absolute. */
int  pg_job_fetch_record_lines_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
/* Device-resident lines of one index contig: *d_text = its first byte, *d_off = uint64 [n_lines + 1] offsets ABSOLUTE
 * in the packed lines. */
int  pg_job_device_record_lines(pg_job* job, uint32_t index_contig, void** d_off, void** d_text, uint64_t* n_lines, uint64_t* n_bytes);
/* Elapsed milliseconds of the kernels of the LAST pg_job_record_lines (lengths, scan, join). */
double pg_job_record_lines_ms(const pg_job* job);
/* Unit entry point: the lines of n_records records of n_members members from host arrays, through the same kernels:
 * member s's record r = text[s][off[s][r] .. off[s][r + 1]); out_off[R + 1] and out[cap] come back.  PG_ERR_INVALID,
 * before any device is asked for: null arrays, an offset array that does not start at 0 or shrinks, n_members == 0,
 * cap below the bound, n_records >= 2^31.  n_records == 0: PG_OK with out_off[0] = 0.  Otherwise PG_ERR_DEVICE without
 * a device: no host fallback. */
int  pg_record_lines_from_text(int device, uint64_t n_records, uint64_t n_members, const uint64_t* const* off, const char* const* text,
                               const uint64_t* prefix_off, const char* prefix, uint64_t* out_off, char* out, uint64_t cap);

/* ------------------------------------------------------------------ *
 *  SLOTTED prefixes: the lines of sampled cohorts.  There every chain is an index contig of its own,
 *  and the fixed columns of the chains of one chromosome differ in one number only: UK, the k-mer count of the record's
 *  bubble in the chain's reduced panel.  A slotted prefix is a prefix and slot[R] with 0 <= slot[r] <= len(prefix[r]);
 *  the line of record r is
 *      prefix[r][0 : slot[r]]  dec(UK)  prefix[r][slot[r] :]  ('\t' text_s[r]) for every member s in order  '\n'
 *  with UK the value pg_job_fetch reports in n_kmers[v] for the bubble v of record r (the plan's rec_var) of the index
 *  contig's FIRST member chain — 0 for a chain without a kept column, 16 bits — and dec its decimal digits without
 *  leading zeros, "0" for 0.  Everything else is the rule above.  slot == NULL: a plain prefix.  A job with at least
 *  one slotted prefix among the index contigs that take part forms all its lines through the slotted instantiation of
 *  pg_record_lines.hip's kernels (a plain prefix gives the same bytes there); a job without one through the plain one.
 *  Not covered: the combined (-a) record families; the phasing column over slotted prefixes (its UK follows another rule).
 * ------------------------------------------------------------------ */
/* pg_record_lines_bound(...) + 5 n_records: an upper bound (UK has at most 5 digits).  Host only. */
uint64_t pg_record_lines_bound_slotted(uint64_t n_records, uint64_t n_members, uint64_t prefix_bytes, uint64_t text_bytes);
/* pg_job_line_prefix with slot[R] (or NULL: pg_job_line_prefix itself).  Also PG_ERR_INVALID: slot[r] > off[r + 1] -
 * off[r]. */
int  pg_job_line_prefix_slotted(pg_job* job, uint32_t index_contig, const uint64_t* off, const char* bytes, const uint32_t* slot, char* err,
                                size_t errlen);
/* ONE prefix, checked once, uploaded once and reference-counted, for every index contig ix with ix % n_contigs ==
 * contig, as pg_job_record_plan_strided shares the record plan; slot may be NULL.  PG_ERR_INVALID: the refusals of
 * pg_job_record_plan_strided (n_contigs == 0, contig >= n_contigs, index contigs that are no multiple of n_contigs),
 * those of pg_job_line_prefix for any member (no record plan; plans of the members that differ in their number of
 * records), and slot[r] > off[r + 1] - off[r].  Nothing is attached on a refusal.  A later pg_job_line_prefix on one
 * member replaces that member's reference alone; a new record plan or index for a member drops its reference.  The
 * lines are stale after it. */
int  pg_job_line_prefix_strided(pg_job* job, uint32_t contig, uint32_t n_contigs, const uint64_t* off, const char* bytes, const uint32_t* slot, char* err,
                                size_t errlen);
/* Unit entry point: pg_record_lines_from_text over a slotted prefix with UK of record r = uk[r], always through
 * the slotted instantiation of pg_record_lines.hip's kernels.  slot == NULL (uk is then not read): a plain prefix, the bytes and offsets of
 * pg_record_lines_from_text.  PG_ERR_INVALID, before any device is asked for: the refusals of pg_record_lines_from_text
 * (cap: below pg_record_lines_bound_slotted with slots, below pg_record_lines_bound without), slot without uk,
 * slot[r] > prefix_off[r + 1] - prefix_off[r]. */
int  pg_record_lines_from_text_slotted(int device, uint64_t n_records, uint64_t n_members, const uint64_t* const* off, const char* const* text,
                                       const uint64_t* prefix_off, const char* prefix, const uint32_t* slot, const uint16_t* uk, uint64_t* out_off,
                                       char* out, uint64_t cap);

/* ------------------------------------------------------------------ *
 *  The PHASING column: `GT:KC` of a run_phasing job per VCF record, formed on the device from the
 *  Viterbi haplotypes the run left there (pangenie_amd/csrc/pg_phase_text.hip; the rule: pg_phase.h), under the record
 *  plans of pg_job_record_plan.  What Graph::write_phasing (reference src/graph.cpp:388-411) prints: for record r of
 *  bubble v with haplotypes H1, H2 (allele ids; 0 at a variant without a column), a_i = map[map_off[r] + H_i]:
 *    allele_i = PG_PHASE_UNDEFINED (printed `.`) if vcf_index[vcf_off[r] + a_i] == 0xFFFF;
 *               else 0 if the record has alleles of undefined sequence and the bubble's result holds no likelihoods (not
 *               run_genotyping, or not a kept column): get_specific_likelihoods maps a haplotype only while it walks
 *               stored genotypes;
 *               else vcf_index[vcf_off[r] + a_i].
 *  The text of a record, no separator, no terminator: `./.` if ignore_imputed and UK == 0, else `allele_1|allele_2`;
 *  then `:` and KC in decimal.  UK and KC follow pg_job_fetch: with run_genotyping and at least one column the bubble's
 *  k-mer count and coverage; otherwise those of the bubbles v < n_columns and 0 beyond (the Viterbi backtrace sets both
 *  at the COLUMN index).  Every record has a text: none is the host's.  The plan calls REF defined whatever it holds.
 *  Everything here is PG_ERR_INVALID for a job without run_phasing, before pg_job_run and after an upload that
 *  invalidated the run; formations run on the job's stream and block; their buffers lie outside the arena, are made by
 *  the first forming and freed by pg_job_destroy (PG_ERR_NOMEM if they do not fit).  A chain whose index contig has no
 *  plan is left out.  Phase, text and lines are stale after a later run, a new plan or a new index, the lines also after
 *  a new prefix: the fetches then answer PG_ERR_INVALID.  Not covered: the combined (-a) record families; slotted and
 *  strided prefixes (the slotted kernel prints UK by the genotyping rule).
 * ------------------------------------------------------------------ */
#ifndef PG_PHASE_DEFINED /* (the same in pangenie_amd/csrc/pg_phase.h) */
#define PG_PHASE_DEFINED
typedef struct pg_phase { uint16_t allele_1, allele_2; } pg_phase;
#define PG_PHASE_UNDEFINED 0xFFFFu   /* the haplotype carries an allele of undefined sequence: printed `.` */
#endif
/* One pg_phase per record of every chain with a plan.  Before the first formation (and after a new plan or index) every
 * allele id is checked on the device against the plans' maps, as pg_job_record_calls checks them: PG_ERR_INVALID. */
int  pg_job_record_phase(pg_job* job, char* err, size_t errlen);
/* Chain `chain`'s records (a chain without a plan has none: out may be NULL) / every chain's, one synchronisation. */
int  pg_job_fetch_record_phase(pg_job* job, uint32_t chain, pg_phase* out, char* err, size_t errlen);
int  pg_job_fetch_record_phase_all(pg_job* job, pg_phase* const* outs, char* err, size_t errlen);
/* Device-resident records of chain `chain` and their number. */
int  pg_job_device_record_phase(pg_job* job, uint32_t chain, void** d_phase, uint64_t* n);
double pg_job_record_phase_ms(const pg_job* job);
/* 13 n_records (255|255:65535): reached exactly when every record is that one.  Host only. */
uint64_t pg_phase_text_bound(uint64_t n_records);
/* Forms the text of every chain with a plan, packed chain after chain; forms the record phase first where it is not
 * formed for this run.  Forming it with another ignore_imputed replaces it. */
int  pg_job_phased_text(pg_job* job, int ignore_imputed, char* err, size_t errlen);
/* record_first / text_first (each [n_chains + 1], either may be NULL): every chain's first record / first byte. */
int  pg_job_phased_text_first(pg_job* job, uint64_t* record_first, uint64_t* text_first, char* err, size_t errlen);
/* As pg_job_fetch_record_text, pg_job_fetch_record_text_packed and pg_job_device_record_text. */
int  pg_job_fetch_phased_text(pg_job* job, uint32_t chain, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_fetch_phased_text_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_device_phased_text(pg_job* job, uint32_t chain, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes);
double pg_job_phased_text_ms(const pg_job* job);
/* Whole lines of the phasing VCF: the second lines family of a job, with prefixes of its own (FORMAT is GT:KC), joined
 * from the phased text by the kernels of pg_job_record_lines (plain prefixes).  Each call is its record-lines sibling
 * over this family: pg_job_line_prefix, pg_job_record_lines (PG_ERR_INVALID unless pg_job_phased_text has been called
 * for this run and these plans), pg_job_record_lines_first, the fetches, the device pointers, the time. */
int  pg_job_phased_line_prefix(pg_job* job, uint32_t index_contig, const uint64_t* off, const char* bytes, char* err, size_t errlen);
int  pg_job_phased_lines(pg_job* job, char* err, size_t errlen);
int  pg_job_phased_lines_first(pg_job* job, uint64_t* n_index_contigs, uint64_t* line_first, uint64_t* byte_first, char* err, size_t errlen);
int  pg_job_fetch_phased_lines(pg_job* job, uint32_t index_contig, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_fetch_phased_lines_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_device_phased_lines(pg_job* job, uint32_t index_contig, void** d_off, void** d_text, uint64_t* n_lines, uint64_t* n_bytes);
double pg_job_phased_lines_ms(const pg_job* job);
/* Unit entry points, through the same kernels; everything is checked on the host first (PG_ERR_INVALID), then
 * PG_ERR_DEVICE without a device: no host fallback.
 * pg_record_phase_from_haplotypes: a plan, hap1 / hap2 [n_variants] allele ids and keyed [n_variants] (the bubble's
 * result holds likelihoods); out[n_records].  Refused: a malformed plan (pg_record_calls_from_bins' checks), null
 * arrays, a haplotype id outside the map of one of its bubble's records.  A plan without variants: PG_OK.
 * pg_phase_text_from_fields: phase[R], kc[R], no_call[R] (or NULL: none); off[R + 1] and text[cap] come back.  Refused:
 * null arrays, n_records >= 2^31, cap < pg_phase_text_bound(R), an allele above 255 that is not PG_PHASE_UNDEFINED (the
 * bound counts on it).  n_records == 0: PG_OK with off[0] = 0. */
int  pg_record_phase_from_haplotypes(int device, const pg_record_plan* plan, const uint16_t* hap1, const uint16_t* hap2, const uint8_t* keyed,
                                     pg_phase* out);
int  pg_phase_text_from_fields(int device, uint64_t n_records, const pg_phase* phase, const uint16_t* kc, const uint8_t* no_call, uint64_t* off,
                               char* text, uint64_t cap);

/* ------------------------------------------------------------------ *
 *  The SAMPLED-PANEL VCF (PanGenie's `-d` output, all that PanGenie-sampling writes) from the device: per VCF
 *  record one `GT` column per selected path of the chain's reduced panel (pangenie_amd/csrc/pg_panel_text.hip; the
 *  rule: pg_panel.h), under the record plan of the chain's index contig.  Cell p of record r:
 *  H = path_allele[v P + p], v the record's bubble and P the chain's paths; a = map[map_off[r] + H];
 *  x = vcf_index[vcf_off[r] + a]; `.` if x == 0xFFFF, else x in decimal.  A record's text = its cells joined by
 *  tabs, no leading tab, no terminator (what Graph::sample_records prints behind `\tGT\t`); every record has one.
 *  pg_panel_text_bound(R, P) = R (4 P - 1) for P >= 1.
 *  pg_job_panel_text needs a record plan on the chain's index contig and NO pg_job_run: it reads the panel, not the
 *  bins, and a later run does not make it stale.  A chain whose index contig has no plan is left out.  The ids are
 *  checked on the device first as pg_job_record_calls does (PG_ERR_INVALID), a path allele outside a record's map is
 *  PG_ERR_INVALID, a chain of more than 64 paths PG_ERR_UNSUPPORTED (the host route is the caller's then), the
 *  buffer outside the arena PG_ERR_NOMEM.  The text is stale after a new plan and after pg_job_upload of a new index
 *  (a new panel): the fetches and device pointers then answer PG_ERR_INVALID, as for an n_bytes that is not the
 *  buffer's.  The fetches are those of pg_job_record_text: per chain (offsets from 0), packed (absolute offsets, all
 *  chains from one copy), device pointers; pg_job_panel_text_first: record_first and / or text_first [n_chains + 1].
 * ------------------------------------------------------------------ */
uint64_t pg_panel_text_bound(uint64_t n_records, uint64_t n_paths);
int  pg_job_panel_text(pg_job* job, char* err, size_t errlen);
int  pg_job_panel_text_first(pg_job* job, uint64_t* record_first, uint64_t* text_first, char* err, size_t errlen);
int  pg_job_fetch_panel_text(pg_job* job, uint32_t chain, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_fetch_panel_text_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_device_panel_text(pg_job* job, uint32_t chain, void** d_off, void** d_text, uint64_t* n_records, uint64_t* n_bytes);
double pg_job_panel_text_ms(const pg_job* job);
/* uk[n_records], n_records = record_first[n_chains]: the UK of every record's line (below), all chains from one copy */
int  pg_job_fetch_panel_uk_packed(pg_job* job, uint16_t* uk, uint64_t n_records, char* err, size_t errlen);
/* Whole lines of the sampled-panel VCF: a third family of prefixes (CHROM .. INFO, `GT`, no trailing tab), joined
 * from the panel text by the kernels of pg_job_record_lines.  Each call is its record-lines sibling over this family.
 * The UK a SLOTTED prefix prints is the panel's own count of the record's bubble, kmer_off[v + 1] - kmer_off[v]
 * (UniqueKmers::size(), what SampledPanel::unique_kmers holds, in 16 bits), which pg_job_panel_text keeps per record
 * — not pg_job_fetch's rule, which answers 0 for a chain without a kept column.  The lines are stale when the text
 * is, after a text formed again and after a new prefix. */
int  pg_job_panel_line_prefix(pg_job* job, uint32_t index_contig, const uint64_t* off, const char* bytes, char* err, size_t errlen);
int  pg_job_panel_line_prefix_slotted(pg_job* job, uint32_t index_contig, const uint64_t* off, const char* bytes, const uint32_t* slot, char* err,
                                      size_t errlen);
int  pg_job_panel_line_prefix_strided(pg_job* job, uint32_t contig, uint32_t n_contigs, const uint64_t* off, const char* bytes, const uint32_t* slot,
                                      char* err, size_t errlen);
int  pg_job_panel_lines(pg_job* job, char* err, size_t errlen);
int  pg_job_panel_lines_first(pg_job* job, uint64_t* n_index_contigs, uint64_t* line_first, uint64_t* byte_first, char* err, size_t errlen);
int  pg_job_fetch_panel_lines(pg_job* job, uint32_t index_contig, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_fetch_panel_lines_packed(pg_job* job, uint64_t* off, char* text, uint64_t n_bytes, char* err, size_t errlen);
int  pg_job_device_panel_lines(pg_job* job, uint32_t index_contig, void** d_off, void** d_text, uint64_t* n_lines, uint64_t* n_bytes);
double pg_job_panel_lines_ms(const pg_job* job);
/* Unit entry point, through the same kernels: a plan and path_allele [n_variants x n_paths] in; off[R + 1] and text[cap]
 * come back.  Everything is checked on the host first — a malformed plan (pg_record_calls_from_bins' checks, 2^31 records
 * or more), null arrays, n_paths == 0, an allele id outside the map of one of its bubble's records, cap below
 * pg_panel_text_bound(R, n_paths): PG_ERR_INVALID; n_paths > 64: PG_ERR_UNSUPPORTED — then PG_ERR_DEVICE without a device:
 * no host fallback.  A plan without variants: PG_OK with off[0] = 0. */
int  pg_panel_text_from_paths(int device, const pg_record_plan* plan, uint32_t n_paths, const uint16_t* path_allele, uint64_t* off, char* text,
                              uint64_t cap);

/* ------------------------------------------------------------------ *
 *  Path subsets: the chains of one contig over different path selections combined on the device, and the calls
 *  from the sums (pangenie_amd/csrc/pg_combine.hip).  The reference's `-a` option genotypes a
 *  chromosome once per subset of paths, adds the subsets' UNNORMALISED likelihoods per genotype
 *  (src/commands.cpp:163-177; GenotypingResult::combine, src/genotypingresult.cpp:193-198) and normalises once.
 *  Chains s = 0 .. S-1 of a GROUP genotype the same index objects; chain s holds key (a <= b) of variant v iff
 *  kept_s[v] && allele_present_s[a] && allele_present_s[b].  The combined map of a variant has the UNION of the
 *  chains' keys (a key held with the value 0 is present), each value ((L_s1 + L_s2) + L_s3) ... over the chains
 *  that hold it IN THE ORDER OF THE GROUP, every addition rounded as the x87 rounds a long double.
 * ------------------------------------------------------------------ */
#ifndef PG_COMBINED_DEFINED /* (the same in pangenie_amd/csrc/pg_combine.h) */
#define PG_COMBINED_DEFINED
typedef struct pg_combined_bin { uint64_t m; int32_t e; uint32_t flags; } pg_combined_bin;
/* value = m * 2^e, m in [2^63, 2^64) or 0 (then e == 0): ldexpl((long double)m, e) is exact */
#define PG_COMBINED_PRESENT  1u   /* the key exists in the combined map                      */
#define PG_COMBINED_DEFERRED 2u   /* present, not formed on the device: add this key on the  */
                                  /* host from the chains' bins (m == 0, e == 0)             */
#endif
/* A key is PG_COMBINED_DEFERRED iff its largest nonzero summand lies below 2^-16300 (the cut of PG_CALL_DEFERRED).
 *
 * The plan: group g = chains[group_off[g] .. group_off[g + 1]), in combine order.  A second plan replaces the first.
 * PG_ERR_INVALID, and nothing is attached: n_groups == 0, an empty group, a chain >= pg_job_n_chains, a chain listed
 * twice (in one group or in two), members whose n_variants, alleles per variant or allele ids differ (checked on the
 * device, against the arrays it holds: sampled panels too), a job without run_genotyping.  The buffers (16 bytes per
 * bin and 8 per variant of every group) lie outside the arena and are freed by pg_job_destroy; PG_ERR_NOMEM if they
 * do not fit. */
int  pg_job_combine_plan(pg_job* job, uint32_t n_groups, const uint32_t* group_off, const uint32_t* chains, char* err, size_t errlen);
/* Combines every group of the plan from the bins of the last pg_job_run (on the job's stream; blocking).  Refusals as
 * pg_job_calls, and PG_ERR_INVALID without a plan.  After an index upload the layout is checked again first. */
int  pg_job_combine(pg_job* job, char* err, size_t errlen);
/* Group `group`'s combined bins, out[geno_off[V]] in the layout of the members' bins (after pg_job_combine of this run). */
int  pg_job_fetch_combined(pg_job* job, uint32_t group, pg_combined_bin* out, char* err, size_t errlen);
/* The same for all groups, outs[n_groups] (NULL allowed for a group without variants): one synchronisation. */
int  pg_job_fetch_combined_all(pg_job* job, pg_combined_bin* const* outs, char* err, size_t errlen);
/* Device-resident combined bins of group `group`: pg_combined_bin [n]. */
int  pg_job_device_combined(pg_job* job, uint32_t group, void** d_bins, uint64_t* n);
/* One pg_call per variant of every group from its combined bins: normalize, get_likeliest_genotype and
 * get_genotype_quality on the combined map, as pg_job_calls on one chain's (allele_1 / allele_2 are allele ids).  A
 * variant with a PG_COMBINED_DEFERRED bin is PG_CALL_DEFERRED.  PG_ERR_INVALID before pg_job_combine of the same run. */
int  pg_job_combined_calls(pg_job* job, char* err, size_t errlen);
int  pg_job_fetch_combined_calls(pg_job* job, uint32_t group, pg_call* out, char* err, size_t errlen);
int  pg_job_fetch_combined_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen);
int  pg_job_device_combined_calls(pg_job* job, uint32_t group, void** d_calls, uint64_t* n);
/* Groups of the job's plan (0 without one). */
uint32_t pg_job_n_groups(const pg_job* job);
/* Elapsed milliseconds of the kernels of the LAST pg_job_combine / pg_job_combined_calls. */
double pg_job_combine_ms(const pg_job* job);
double pg_job_combined_calls_ms(const pg_job* job);
/* Unit entry points, through the same kernels; PG_ERR_DEVICE without a device, no host fallback.
 * pg_combine_bins: n_chains >= 1 chains over one layout (allele_off [V+1]); kept[s] [V], allele_present[s] [sumA],
 * lik[s] / lik_exp[s] [sum A (A + 1) / 2] of chain s, combined in the order given; out[sum A (A + 1) / 2]. */
int  pg_combine_bins(int device, uint32_t n_variants, const uint32_t* allele_off, uint32_t n_chains,
                     const uint8_t* const* kept, const uint8_t* const* allele_present,
                     const double* const* lik, const int32_t* const* lik_exp, pg_combined_bin* out);
/* pg_calls_from_combined: the calls of n_variants variants from their combined bins; out[V].  PG_ERR_INVALID for a bin
 * that is no pg_combined_bin: m neither 0 nor normalised, unknown flags, a value without PG_COMBINED_PRESENT. */
int  pg_calls_from_combined(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id,
                            const pg_combined_bin* bins, pg_call* out);

/* ---------------------------------------------------------------------------------------------------------------
 *  Path subsets to VCF lines: GT, GQ and the GL column per VCF RECORD from the combined bins
 *  (pangenie_amd/csrc/pg_combine_records.hip).  For record r of variant v of group g, under the
 *  record plan of the index contig of the group's FIRST chain (pg_job_record_plan / pg_job_record_plan_strided), the
 *  fields are what Graph::write_genotypes prints for GenotypingResult::combine of the members in group order:
 *  normalize() of the combined map (the bins with PG_COMBINED_PRESENT, value m 2^e), the fold onto the record's alleles,
 *  an empty result as L(0/0) = 1, get_specific_likelihoods over the defined alleles, then likeliest genotype and quality
 *  (pg_call: allele_1 <= allele_2 are GT numbers, PG_CALL_EMPTY as in pg_job_record_calls) and setprecision(4) of
 *  log10 L (pg_gl, laid out by pg_record_gl_offsets).  A variant with a PG_COMBINED_DEFERRED bin makes every one of
 *  its records PG_CALL_DEFERRED and every one of its values PG_GL_DEFERRED; the other deferral rules are those of
 *  pg_job_record_calls / pg_job_record_gl.
 *  A group whose first chain's index contig has no plan is left out (no records); the other members need none.
 *  Both calls run on the job's stream and block; their buffers lie outside the arena, allocated on first use
 *  (PG_ERR_NOMEM).  PG_ERR_INVALID without a combine plan, before pg_job_combine of the same run, when no group has
 *  a plan, and for an allele id of a group's first chain outside a map of its plan (checked on the device before the
 *  first formation and again after a new record plan, combine plan, index upload or pg_job_combine; the message names
 *  group and variant).  Each of those four also invalidates what was formed.
 * --------------------------------------------------------------------------------------------------------------- */
int  pg_job_combined_record_calls(pg_job* job, char* err, size_t errlen);
int  pg_job_combined_record_gl(pg_job* job, char* err, size_t errlen);
/* Group `group`'s records / values (a group without a plan has none: out may be NULL). */
int  pg_job_fetch_combined_record_calls(pg_job* job, uint32_t group, pg_call* out, char* err, size_t errlen);
int  pg_job_fetch_combined_record_gl(pg_job* job, uint32_t group, pg_gl* out, char* err, size_t errlen);
/* Every group's, outs[g] (NULL allowed for a group without records), copies queued on the job's stream, one wait. */
int  pg_job_fetch_combined_record_calls_all(pg_job* job, pg_call* const* outs, char* err, size_t errlen);
int  pg_job_fetch_combined_record_gl_all(pg_job* job, pg_gl* const* outs, char* err, size_t errlen);
/* Device-resident records / values of group `group` and their number. */
int  pg_job_device_combined_record_calls(pg_job* job, uint32_t group, void** d_calls, uint64_t* n);
int  pg_job_device_combined_record_gl(pg_job* job, uint32_t group, void** d_gl, uint64_t* n);
/* Elapsed milliseconds of the kernels of the LAST formation. */
double pg_job_combined_record_calls_ms(const pg_job* job);
double pg_job_combined_record_gl_ms(const pg_job* job);
/* Unit entry points, through the same kernels: one contig's combined bins (as pg_calls_from_combined takes them) and a
 * plan; out[plan->n_records] records / out[gl_off[n_records]] values.  Checked on the host first: the layout, the plan
 * (PG_ERR_INVALID; PG_ERR_UNSUPPORTED for a record of more than 256 alleles), every allele id against the plan's maps,
 * the bins, `out`; then PG_ERR_DEVICE without a device.  No host fallback. */
int  pg_record_calls_from_combined(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id,
                                   const pg_combined_bin* bins, const pg_record_plan* plan, pg_call* out);
int  pg_record_gl_from_combined(int device, uint32_t n_variants, const uint32_t* allele_off, const uint16_t* allele_id,
                                const pg_combined_bin* bins, const pg_record_plan* plan, pg_gl* out);

#ifdef __cplusplus
}
#endif
#endif /* PANGENIE_HMM_H */
