/*
 * pangenie_kmers.h — C ABI of the device k-mer counter: the counts of a GIVEN set of k-mers in a
 * sample's reads, the step in front of fill_read_kmercounts, with the table in HBM and the reads streamed through the
 * GPU.  Same semantics as pangenie::TargetedKmerCounter (pangenie_amd/host/kmer_counts.hpp):
 *
 *  - k = 1..32.  A k-mer is coded 2 bits a letter (A, C, G, T = 0..3, either letter case, first letter in the highest
 *    bits) and counted under the smaller of its code and its reverse complement's code (the canonical code).
 *  - "text" is any byte buffer: every byte outside ACGTacgt ends the current run of windows, so sequences back to back
 *    with one newline after each need no offsets.
 *  - every window of k valid letters is one "window seen"; if its canonical code is registered its count goes up by
 *    one.  Counts are 64-bit integers: equal, not close, to what the host counters give.
 *
 * The table: open addressing, 16-byte slots {key, count}, capacity max(16, 2 * registered codes + 1) (repeats
 * included, as on the host), a code starts probing at the high 64 bits of mix64(code) * capacity and probes on
 * linearly; mix64 is the splitmix64 finaliser.  PG_KMER_NOT_REGISTERED marks an empty slot (it is never a canonical
 * code: the reverse complement of all-T is all-A = 0).  pg_kmer_counter_table hands that layout to the host as it is.
 *
 * A handle is used from one thread at a time.  Error codes are those of pangenie_hmm.h; the text of the calling
 * thread's last error is at pg_kmer_last_error().
 */
#ifndef PANGENIE_KMERS_H
#define PANGENIE_KMERS_H

#include "pangenie_hmm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_KMER_NOT_REGISTERED (~0ull)

typedef struct pg_kmer_counter pg_kmer_counter;

/* PG_ERR_INVALID for k outside 1..32 or a null `out`, decided before any device call; PG_ERR_DEVICE without a GPU. */
int pg_kmer_counter_new(uint32_t k, int device, pg_kmer_counter** out);
int pg_kmer_counter_destroy(pg_kmer_counter* h);
/* register n canonical codes formed by the host (the `_kmers.tsv.gz` route); a code that is not below 4^k is
 * PG_ERR_INVALID (nothing of the call is registered then) */
int pg_kmer_counter_add_codes(pg_kmer_counter* h, const uint64_t* codes, uint64_t n);
/* register every window of a text, coded on the device (the `_path_segments.fasta` route); *windows (may be NULL) =
 * how many were registered by this call, repeats included */
int pg_kmer_counter_add_text(pg_kmer_counter* h, const char* text, uint64_t bytes, uint64_t* windows);
/* build the table on the device (compare-and-swap insertion; repeats collapse).  Implied by the first count.
 * PG_ERR_NOMEM when the table does not fit: the call never shrinks it on its own. */
int pg_kmer_counter_freeze(pg_kmer_counter* h);
/* count a host buffer: copied through pinned staging buffers on the counter's own stream; returns once the last piece
 * is submitted, not once it is counted.  Counts of all calls add up.  Registering afterwards is PG_ERR_INVALID. */
int pg_kmer_counter_count(pg_kmer_counter* h, const char* text, uint64_t bytes);
/* The same without the copy into the staging buffer: acquire waits for a free pinned buffer and hands it out
 * (*capacity bytes), the caller fills it while earlier buffers are copied and counted, submit counts its first `bytes`
 * bytes.  One buffer is out at a time; a buffer is one text of its own (windows do not run across buffers). */
int pg_kmer_counter_acquire(pg_kmer_counter* h, char** buffer, uint64_t* capacity);
int pg_kmer_counter_submit(pg_kmer_counter* h, uint64_t bytes);
/* everything submitted so far is counted */
int pg_kmer_counter_sync(pg_kmer_counter* h);
/* counts[i] = count of canonical code codes[i], gathered on the device in one launch; a code that was never registered
 * answers PG_KMER_NOT_REGISTERED, never a silent 0.  Freezes and syncs. */
int pg_kmer_counter_lookup(pg_kmer_counter* h, const uint64_t* codes, uint64_t n, uint64_t* counts);
/* distinct registered codes (freezes), windows seen (syncs); either pointer may be NULL */
int pg_kmer_counter_stats(pg_kmer_counter* h, uint64_t* targets, uint64_t* windows);
/* out[c] = registered k-mers seen c times, c = 1..max_count; out[0] = 0, larger counts are left out
 * (TargetedKmerCounter::abundance_histogram).  out holds max_count + 1 entries. */
int pg_kmer_counter_histogram(pg_kmer_counter* h, uint64_t max_count, uint64_t* out);
/* zero counts and windows seen, keep the table: the next sample of a cohort over the same index */
int pg_kmer_counter_reset_counts(pg_kmer_counter* h);
/* slots of the table (freezes) */
int pg_kmer_counter_capacity(pg_kmer_counter* h, uint64_t* capacity);
/* the whole table to the host, in the layout described above: slots[2 * i] = key, slots[2 * i + 1] = count of slot i;
 * `capacity` must be what pg_kmer_counter_capacity answers.  Syncs. */
int pg_kmer_counter_table(pg_kmer_counter* h, uint64_t* slots, uint64_t capacity);
/* Measurement: the counting kernel alone on a text already resident in HBM — uploaded once, counted `repeats` times,
 * ms[r] = device time of repeat r (events).  The counts of all repeats are added like any others. */
int pg_kmer_counter_count_resident(pg_kmer_counter* h, const char* text, uint64_t bytes, uint32_t repeats, double* ms);
/* text positions a workgroup of the counting kernel takes (tests place separators and buffer ends around it) */
uint32_t pg_kmer_tile_bytes(void);
const char* pg_kmer_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PANGENIE_KMERS_H */
