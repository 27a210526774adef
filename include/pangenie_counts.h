/*
 * pangenie_counts.h — C ABI of the count plan: the step between the device k-mer counter
 * (pangenie_kmers.h) and a cohort job (pangenie_hmm.h), i.e. pangenie::fill_read_kmercounts with the table left in HBM.
 *
 * Which k-mers a variant asks about, in which order, and which of them are flanking k-mers is a property of the INDEX:
 * a plan takes those lists once, resolves every code to its slot of the counter's table once, and keeps the slot indices
 * on the device.  What a SAMPLE adds is the counts: a fill is one gather kernel over the table that writes
 *
 *   kmer_count[c][i] = (uint16_t) count(kmer_code[c][i])                      (truncating cast, no saturation)
 *   coverage[c][v]   = (uint16_t) windowed_mean(counts of the flanking k-mers of variant v, kmer_coverage)
 *
 * windowed_mean: lowest = kmer_coverage / 4, highest = kmer_coverage * 4 (64-bit arithmetic), the integer mean of the
 * counts inside [lowest, highest] when there is at least one and their sum is not 0, else kmer_coverage.  A variant
 * without flanking k-mers gets kmer_coverage.  Equal, not close, to what fill_read_kmercounts writes.
 *
 * A code equal to PG_KMER_NOT_REGISTERED (a k-mer with a letter outside ACGT) always counts 0.  A valid code that is not
 * in the table counts 0 in a plan made with unregistered_counts_zero; without it pg_count_plan_new fails.
 *
 * A plan keeps a pointer to its counter: the counter must outlive it, and both are used from one thread at a time.
 * Error codes are those of pangenie_hmm.h; the text of the calling thread's last error is at pg_kmer_last_error().
 */
#ifndef PANGENIE_COUNTS_H
#define PANGENIE_COUNTS_H

#include "pangenie_kmers.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pg_count_plan pg_count_plan;

/* one contig of the index: host arrays, read during pg_count_plan_new only.  Offsets start at 0 and never decrease.
 * A contig without variants, k-mers or flanking k-mers is legal; the arrays it does not need may be NULL. */
typedef struct pg_count_contig {
    uint32_t        n_variants;
    const uint32_t* kmer_off;    /* [V + 1]  unique k-mers of variant v: [kmer_off[v], kmer_off[v + 1])              */
    const uint64_t* kmer_code;   /* [kmer_off[V]]  canonical codes, in the k-mer order of the variant's UniqueKmers  */
    const uint64_t* flank_off;   /* [V + 1]  flanking k-mers of variant v                                            */
    const uint64_t* flank_code;  /* [flank_off[V]]                                                                   */
} pg_count_contig;

/* Freezes the counter, uploads the codes and resolves them against its table.  PG_ERR_INVALID, decided on the host
 * before any device call: null `counter` / `out` / `contigs`, null arrays a contig needs, offsets that do not start at 0
 * or decrease, a code that is neither PG_KMER_NOT_REGISTERED nor below 4^k.  PG_ERR_INVALID after the resolve: a plan
 * without unregistered_counts_zero met a valid code that is not in the table; pg_kmer_last_error() names contig, variant
 * and position of the first one in index order. */
int pg_count_plan_new(pg_kmer_counter* counter, uint32_t n_contigs, const pg_count_contig* contigs,
                      int unregistered_counts_zero, pg_count_plan** out);
int pg_count_plan_destroy(pg_count_plan* plan);
/* Per sample.  All three wait until everything submitted to the counter is counted, run ONE kernel for all contigs and
 * return when its results are where they go.  kmer_count[c] / coverage[c] take kmer_off[V] / V entries of contig c
 * (an entry of a contig that has none may be NULL).
 *  _host:   host arrays.
 *  _device: arrays in the memory of the counter's device (hipMalloc; every array is asked about with
 *           hipPointerGetAttributes and anything else, managed memory included, is PG_ERR_INVALID: a host pointer
 *           would fault the kernel). */
int pg_count_plan_fill_host(pg_count_plan* plan, uint64_t kmer_coverage, uint16_t* const* kmer_count, uint16_t* const* coverage);
int pg_count_plan_fill_device(pg_count_plan* plan, uint64_t kmer_coverage, uint16_t* const* d_kmer_count, uint16_t* const* d_coverage);
/* _job: straight into the per-sample arrays of chains sample * n_contigs + c of a cohort job (pg_cohort_new) on the
 * counter's device — the set the next pg_job_run reads; the job's host copy of those chains' coverage is refreshed
 * (2 bytes per variant come back).  The job's contig c must have the plan's n_variants and kmer_off.  Refused between
 * pg_job_upload_begin and pg_job_upload_end.  Like pg_job_upload_end it invalidates the results of the last run:
 * pg_job_fetch answers PG_ERR_INVALID until the next pg_job_run (also when the fill itself fails after its checks).  After it, pg_job_run + pg_job_fetch give what
 * pg_job_upload(job, NULL, samples) with the arrays pg_count_plan_fill_host writes gives. */
int pg_count_plan_fill_job(pg_count_plan* plan, uint64_t kmer_coverage, pg_job* job, uint32_t sample, char* err, size_t errlen);
/* n_kmers / n_flanks: entries of all contigs; unresolved: valid codes that are not in the table (they count 0; always 0
 * for a plan without unregistered_counts_zero); device_bytes: what the plan holds in HBM.  Any pointer may be NULL. */
int pg_count_plan_stats(const pg_count_plan* plan, uint64_t* n_kmers, uint64_t* n_flanks, uint64_t* unresolved, uint64_t* device_bytes);
/* device time of the kernel of the last fill in ms (events); 0 before the first */
double pg_count_plan_last_fill_ms(const pg_count_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* PANGENIE_COUNTS_H */
