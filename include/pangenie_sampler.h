/*
 * pangenie_sampler.h — C ABI of the MI355X-native HaplotypeSampler: the step the
 * reference runs right before the genotyping HMM on large panels (default above 100 paths,
 * reference src/commands.cpp:799-803): `size` passes of an integer (phred-cost) Viterbi over the H
 * panel paths pick a mosaic panel of `size` paths per variant (reference
 * src/haplotypesampler.cpp:20-77, :110-294; emission costs src/samplingemissions.cpp:9-45,
 * transition cost src/samplingtransitions.cpp:5-23).
 *
 * Input = the same flat batch as the genotyping path (include/pangenie_hmm.h: pg_contig_batch) over
 * ALL paths of the panel (n_paths = UniqueKmers::get_nr_paths()).  Everything is integer work: results
 * (sampled path ids, best scores) are bit-exact with the reference.  Transition costs are formed on the
 * host exactly as the reference forms them (long double, then truncation); emission costs on the host by
 * pg_sampler_run[_batch] / pg_sampler_then_job and on the device by pg_sampler_cohort_new, from one table
 * of the same float expression (exact: an allele has at most 32 k-mers); the passes themselves — column
 * minima, DP update, backtrace, penalties — run on the GPU.
 */
#ifndef PANGENIE_SAMPLER_H
#define PANGENIE_SAMPLER_H

#include "pangenie_hmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SamplingEmissions ctor (src/samplingemissions.cpp:9-37) for every allele slot of every variant:
 * 50 for an undefined allele, (unsigned short)(-10 log10(fraction of the allele's k-mers with a read
 * count >= 3)), 25 if none is present; an allele without k-mers has fraction 1 -> 0.  Host. */
int pg_sampler_emission_costs(const pg_contig_batch* panel, uint16_t* cost_sumA);
/* SamplingTransitions ctor (src/samplingtransitions.cpp:5-14): (unsigned int)(-10 log10 q),
 * q = (1 - e^(-d/H)) / H in long double.  Host. */
uint32_t pg_sampler_transition_cost(uint64_t from_pos, uint64_t to_pos, double recombrate,
                                    uint32_t nr_paths, long double effective_N);
/* HaplotypeSampler::get_column_minima (src/haplotypesampler.cpp:79-107) on the device: smallest and
 * second smallest unmasked entry, ties to the smaller index.  out4 = {first_id, second_id, first_val,
 * second_val} (ids 0xFFFFFFFF when there is none).  Unit-level entry for the reference's own tests. */
int pg_sampler_column_minima(const uint32_t* column, const uint8_t* mask, uint32_t n, int device,
                             uint32_t out4[4], char* err, size_t errlen);
/* HaplotypeSampler ctor body for one contig: `size` Viterbi passes.  sampled_paths[s * V + v] = path id
 * picked by pass s at variant v (SampledPaths::sampled_paths, src/haplotypesampler.hpp:17-20);
 * best_scores[s] = DP score of pass s (may be NULL).  The caller applies UniqueKmers::update_paths
 * (and appends the reference path 0 when add_reference is set) as the reference's ctor does
 * (src/haplotypesampler.cpp:44, :296-309). */
int pg_sampler_run(const pg_contig_batch* panel, uint32_t size, double recombrate, long double effective_N,
                   uint16_t allele_penalty, int device, uint32_t* sampled_paths, uint32_t* best_scores,
                   char* err, size_t errlen);
/* The same for several contigs at once — one workgroup per contig and pass, which is how the sampler fills
 * more than one CU (the passes and the columns of a contig are sequential by construction).  panels[g],
 * sampled_paths[g] ([size * V_g]) and best_scores[g] ([size], the array or single entries may be NULL)
 * belong to contig g; contigs without variants are skipped. */
int pg_sampler_run_batch(const pg_contig_batch* panels, uint32_t n_contigs, uint32_t size, double recombrate,
                         long double effective_N, uint16_t allele_penalty, int device,
                         uint32_t* const* sampled_paths, uint32_t* const* best_scores, char* err, size_t errlen);
/* Sampler -> UniqueKmers::update_paths -> genotyping job with the panel staying on the device (the reference's
 * constructor tail, src/haplotypesampler.cpp:44, :296-309; src/biallelicuniquekmers.cpp:223-260,
 * src/multiallelicuniquekmers.cpp:195-232, followed by run_genotyping on the sampled panel, src/commands.cpp:138-152):
 * `size` passes over every contig of `panels`, then the panel reduced — on the GPU — to the sampled paths (+ the
 * reference path 0 when add_reference), the alleles they carry and the k-mers on those alleles, and a resident job
 * (include/pangenie_hmm.h: pg_job_run / pg_job_fetch) over the reduced panel: chain g = contig g, size (+ 1) paths.
 * Only two counts per variant travel to the host (the job's memory is planned from them).  sampled_paths /
 * best_scores as in pg_sampler_run_batch, or NULL.  The reduced panel (its allele ids give the genotype bins their
 * meaning) is read back with pg_job_fetch_panel.  At most 1024 kept paths, 1024 alleles and 2048 k-mers per variant. */
int pg_sampler_then_job(const pg_contig_batch* panels, uint32_t n_contigs, uint32_t size, int add_reference,
                        double sampling_recombrate, long double sampling_effective_N, uint16_t allele_penalty,
                        const pg_table* table, const pg_hmm_params* params, int device,
                        uint32_t* const* sampled_paths, uint32_t* const* best_scores,
                        pg_job** out_job, char* err, size_t errlen);
/* Sampled cohort: pg_sampler_then_job for n_samples samples over ONE index (the reference's per-sample sequence
 * fill_read_kmercounts -> HaplotypeSampler -> HMM on large panels, src/commands.cpp:118-152, run for a whole cohort).
 * Chain s * n_contigs + c of *out_job (the numbering of pg_cohort_new) is, bit for bit in every output — sampled paths, best
 * scores, the reduced panel (pg_job_fetch_panel), lik / lik_exp / kept / n_kmers / coverage / n_columns and, with
 * params->run_phasing, haplotype_1 / haplotype_2 — what pg_sampler_then_job gives for index[c] with
 * kmer_count = samples[s].kmer_count[c] and coverage = samples[s].coverage[c].  index[c].kmer_count / .coverage are ignored.
 * The index arrays cross PCIe once and the transition costs and slot tables are formed once per contig, shared by every
 * sample; per sample only the k-mer counts are uploaded (the coverage goes to the job), and its emission costs are formed
 * on the device.  sampled_paths[s * n_contigs + c] ([size * V_c]) / best_scores[...] ([size]): the array or single entries
 * may be NULL.  Errors: PG_ERR_INVALID for a null argument, n_samples == 0, a sample whose arrays are NULL for a contig with
 * k-mers (coverage: with variants), size < 1 or size >= n_paths; PG_ERR_UNSUPPORTED for the limits of pg_sampler_then_job
 * and more than 65535 chains with variants; PG_ERR_NOMEM when the batch does not fit the device — the message states the
 * bytes needed and the caller splits the samples (the call never splits them itself). */
int pg_sampler_cohort_new(int device, uint32_t n_contigs, const pg_contig_batch* index,
                          uint32_t n_samples, const pg_sample_counts* samples,
                          uint32_t size, int add_reference,
                          double sampling_recombrate, long double sampling_effective_N, uint16_t allele_penalty,
                          const pg_table* table, const pg_hmm_params* params,
                          uint32_t* const* sampled_paths,   /* [n_samples*n_contigs] -> [size*V_c], or NULL */
                          uint32_t* const* best_scores,     /* [n_samples*n_contigs] -> [size],     or NULL */
                          pg_job** out_job, char* err, size_t errlen);
/* Device-resident per-sample arrays of a sampled cohort in the making: for each of n_samples samples and n_contigs contigs
 * one uint16_t[n_kmers[c]] and one uint16_t[n_variants[c]], all in ONE allocation on `device` (every array 256-byte aligned;
 * a contig without k-mers or variants gets a valid, non-null, zero-length slice).  Nothing is written to them here: a count
 * plan's device fill, a kernel or a D2D copy of the caller fills them.  PG_ERR_INVALID (decided before any device call) for a
 * null argument, n_contigs == 0 or n_samples == 0; PG_ERR_DEVICE without a GPU; PG_ERR_NOMEM — after the one-shot arena pool
 * was emptied — with the bytes needed in the message: fewer samples per handle is the caller's remedy. */
typedef struct pg_sampler_counts pg_sampler_counts;
int pg_sampler_counts_new(int device, uint32_t n_contigs, const uint64_t* n_kmers, const uint32_t* n_variants,
                          uint32_t n_samples, pg_sampler_counts** out, char* err, size_t errlen);
/* NULL is PG_OK */
int pg_sampler_counts_destroy(pg_sampler_counts* h);
/* The two pointer tables ([n_contigs] each, owned by the handle, valid until it is destroyed) of one sample: what a device
 * fill of the count plan (include/pangenie_counts.h) takes as d_kmer_count / d_coverage, and what a pg_sample_counts row of
 * pg_sampler_cohort_new_device points at.  Either output may be NULL.  PG_ERR_INVALID for sample >= n_samples. */
int pg_sampler_counts_rows(const pg_sampler_counts* h, uint32_t sample, uint16_t* const** d_kmer_count, uint16_t* const** d_coverage,
                           char* err, size_t errlen);
/* pg_sampler_cohort_new with every d_samples[s].kmer_count[c] AND d_samples[s].coverage[c] in the memory of `device` (the
 * two pointer tables of a row are host arrays, as before).  Every output is bit for bit what pg_sampler_cohort_new gives for
 * host copies of the same arrays; limits and error codes are its own.  The count arrays are read in place — no copy of them
 * is made and the call's per-chain memory no longer holds them —, so they must stay valid and unwritten until the call
 * returns; the returned job does not reference them.  The coverage (which pg_job_new takes from the host) is gathered by one
 * kernel into one buffer and comes back with ONE D2H copy of 2 * V bytes per sample and contig.  Before any allocation or
 * launch every array that is needed (kmer_count: contig with k-mers; coverage: contig with variants) is asked about with
 * hipPointerGetAttributes: anything that is not device memory of `device` — a host pointer, managed memory — is PG_ERR_INVALID
 * with sample, contig and array named (a host pointer would fault a kernel).  Null-argument checks come first and need no
 * device.  After the call pg_sampler_last_h2d_bytes answers [1] == 0 and [0] as after pg_sampler_cohort_new;
 * pg_sampler_last_phase_ms[1] covers the index upload alone and [4] includes the read-back of the coverage. */
int pg_sampler_cohort_new_device(int device, uint32_t n_contigs, const pg_contig_batch* index,
                                 uint32_t n_samples, const pg_sample_counts* d_samples,
                                 uint32_t size, int add_reference,
                                 double sampling_recombrate, long double sampling_effective_N, uint16_t allele_penalty,
                                 const pg_table* table, const pg_hmm_params* params,
                                 uint32_t* const* sampled_paths,   /* [n_samples*n_contigs] -> [size*V_c], or NULL */
                                 uint32_t* const* best_scores,     /* [n_samples*n_contigs] -> [size],     or NULL */
                                 pg_job** out_job, char* err, size_t errlen);
/* H2D bytes of the last pg_sampler_cohort_new[_device] / pg_sampler_then_job of this thread: [0] index arrays, [1] per-sample
 * arrays (cohort: the k-mer counts alone, 2 * sumK per sample and contig, 0 for _device; pg_sampler_then_job: the counts and the
 * emission costs the host formed from them).  Pointer tables and the reduced panel's offsets are not counted; neither is what
 * pg_job_new uploads itself (the coverage). */
int pg_sampler_last_h2d_bytes(uint64_t out2[2]);
/* Wall / kernel milliseconds of the last pg_sampler_cohort_new[_device] of this thread: [0] host preparation (checks, transition
 * costs, plan), [1] H2D uploads, [2] emission cost kernel (hipEvents), [3] slot tables and their per-chain copies
 * (hipEvents), [4] the passes incl. the read-back of sampled paths, [5] the panel reduction, [6] pg_job_new, [7] the call. */
int pg_sampler_last_phase_ms(double out8[8]);
/* Kernel milliseconds of the last pg_sampler_run[_batch] / pg_sampler_cohort_new of the calling thread, summed over the passes:
 * [0] cost expansion, [1] forward passes, [2] backtraces; *kernel (may be NULL) = waves per workgroup of
 * the relative-value kernel, 0 when the general (saturating) kernel ran. */
int pg_sampler_last_ms(double out3[3], int* kernel);

#ifdef __cplusplus
}
#endif
#endif /* PANGENIE_SAMPLER_H */
