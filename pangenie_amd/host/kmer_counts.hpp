// kmer_counts.hpp — the step that turns an index into a sample's input: read k-mer counts and local coverage of every
// variant (reference fill_read_kmercounts, src/commands.cpp:74-139; src/kmerparser.cpp; src/kmercounter.hpp) —
// SURVEY.md §8(f)-3.  Host code (hash lookups and text parsing), except DeviceKmerCounter: the same counts with the table
// and the counting on the GPU (include/pangenie_kmers.h), the reader alone on the host.
//
// The reference's count source is Jellyfish (third party, pinned jellyfish=2.2.10 in environment.yml; not in this
// image): JellyfishCounter runs `mer_counter` over the read file with canonical = true (src/jellyfishcounter.cpp:26-49),
// i.e. every window of k letters over {A,C,G,T} of every read is counted under the lexicographically smaller of the
// k-mer and its reverse complement; windows containing any other letter are skipped.  ExactKmerCounter restates that
// with an exact hash map of EVERY k-mer of the reads — for small inputs (tests, regions); TargetedKmerCounter counts only
// the k-mers the index asks about (memory proportional to the index, not to the reads; plain or gzipped reads, worker
// threads) — the same numbers for those k-mers, for read sets of any size; k <= 32.
// The k-mer abundance peak (`kmer_coverage`) is an ARGUMENT here: finding it (the reference's Histogram /
// compute_kmer_coverage over Jellyfish's histogram) is upstream of this path and out of scope.
// Pinned on the reference's own fixtures: tests/data/index_UniqueKmersMap.cereal + index_chr1_kmers.tsv.gz +
// region-reads.fa must give tests/data/region_UniqueKmersList.cereal (what tests/CommandsTest.cpp:59-93 feeds its HMM).
#pragma once

#include <atomic>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <vector>

#include "cereal_io.hpp"
#include "graph_io.hpp"

namespace pangenie {

/** reference src/kmercounter.hpp:8-24 */
class KmerCounter {
public:
    virtual ~KmerCounter() {}
    /** abundance of the given k-mer (canonical representation is used) */
    virtual size_t getKmerAbundance(std::string kmer) = 0;
};

/** exact canonical k-mer counts of a FASTA / FASTQ file (see above) */
class ExactKmerCounter : public KmerCounter {
public:
    ExactKmerCounter(const std::string& readfile, size_t kmer_size);
    size_t getKmerAbundance(std::string kmer) override;
    size_t distinct_kmers() const { return filled_; }

private:
    void add_sequence(const std::string& seq);
    bool encode_canonical(const char* s, uint64_t& code) const;
    void bump(uint64_t code);
    void grow();
    // canonical code -> count: open addressing with linear probing, 12 bytes a slot, doubled at 60 % load (a graph's or a
    // region's worth of k-mers: tens of millions of entries, where a node-based map spends its time in the allocator)
    static constexpr uint64_t kFree = ~0ull;   // (never a canonical code: the reverse complement of all-T is all-A = 0)
    size_t k_;
    std::vector<uint64_t> keys_;
    std::vector<uint32_t> seen_;     // saturates at 2^32 - 1
    size_t filled_ = 0;
};

/** Counts of a GIVEN set of k-mers in read files of any size.  fill_read_kmercounts only ever asks for the unique and
 *  the flanking k-mers listed in the `_kmers.tsv.gz` tables of the index, so those are registered first
 *  (add_targets_from_table for every chromosome), then the reads are streamed once (count(): FASTA / FASTQ, plain or
 *  gzipped; one reader, `threads` counting workers) and every window that is a registered k-mer is counted under its
 *  canonical code in an open-addressing table.  getKmerAbundance of a k-mer that was never registered throws (a silent 0
 *  would be a wrong count).  Same counts as ExactKmerCounter / the reference's Jellyfish pass for registered k-mers. */
class TargetedKmerCounter : public KmerCounter {
public:
    /** `unregistered_counts_zero`: what getKmerAbundance does for a k-mer that was never registered — false (default): throw;
     *  true: return 0, which is what the reference's graph-only JellyfishCounter answers (tests/KmerCounterTest.cpp:21-32) */
    explicit TargetedKmerCounter(size_t kmer_size, bool unregistered_counts_zero = false);
    /** register a k-mer (any orientation); k-mers with letters outside ACGT can never be counted and are ignored */
    void add_target(std::string_view kmer);
    /** register every unique and flanking k-mer of a `<prefix>_<chromosome>_kmers.tsv(.gz)` table; returns how many rows */
    size_t add_targets_from_table(const std::string& kmers_tsv_gz);
    /** register every window of a FASTA / FASTQ file — `<prefix>_path_segments.fasta` makes this counter the reference's
     *  default count source (JellyfishCounter(readfile, {segment_file}, ...), src/jellyfishcounter.cpp:51-84: only k-mers of
     *  the graph are counted); returns how many windows were registered (with repeats) */
    size_t add_targets_from_sequences(const std::string& fasta);
    /** register every window of a sequence held in memory */
    void add_targets_of(std::string_view sequence);
    /** stream a read file and count; may be called for several files (counts add up).  No targets may be added afterwards. */
    void count(const std::string& readfile, unsigned threads = 1);
    size_t getKmerAbundance(std::string kmer) override;
    size_t targets() const { return n_targets_; }
    /** how many registered k-mers were seen c times, c = 1..max_count (index 0 stays 0, larger counts are left out) — the
     *  numbers the reference's JellyfishCounter::computeHistogram collects (src/jellyfishcounter.cpp:119-126) before it
     *  looks for the abundance peak; the peak rule itself is not part of this build (see above) */
    std::vector<size_t> abundance_histogram(size_t max_count);
    size_t kmers_seen() const { return windows_; }   // windows over ACGT of all reads streamed so far

private:
    bool encode_canonical(const char* s, uint64_t& code) const;
    void freeze(unsigned threads = 1);
    size_t find(uint64_t code) const;   // slot, or npos
    void count_sequence(const char* s, size_t n, uint64_t& windows);
    static constexpr uint64_t kEmpty = ~0ull;   // (never a canonical code: the reverse complement of all-T is all-A = 0)
    size_t k_;
    std::vector<uint64_t> pending_;     // codes registered before the table is built
    struct Slot { uint64_t key, count; };
    // (resize() of this vector leaves new slots untouched — freeze() fills them from its workers, so that the pages of a
    // table of gigabytes are first touched in parallel)
    template <class T> struct RawAllocator : std::allocator<T> {
        template <class U> struct rebind { using other = RawAllocator<U>; };
        template <class U, class... A> void construct(U* p, A&&... a) {
            if constexpr (sizeof...(A) == 0) ::new ((void*)p) U; else ::new ((void*)p) U(std::forward<A>(a)...);
        }
    };
    std::vector<Slot, RawAllocator<Slot>> slots_;   // open addressing, power-of-two size, linear probing
    size_t n_targets_ = 0;
    uint64_t windows_ = 0;
    bool frozen_ = false;
    bool lenient_ = false;
};

/** TargetedKmerCounter with the table in HBM and the counting on the GPU (include/pangenie_kmers.h): the same
 *  public interface, the same counts.  The reader stays on the host (gz, FASTA / FASTQ grammar) and writes the sequences of a
 *  batch straight into a pinned staging buffer, which the device copies and counts while the reader fills the next one.
 *  After counting, getKmerAbundance answers from a host copy of the table fetched once (on the first call, which may come
 *  from any thread), so fill_read_kmercounts[_all] work with it unchanged.  Everything else is called from one thread. */
class DeviceKmerCounter : public KmerCounter {
public:
    explicit DeviceKmerCounter(size_t kmer_size, bool unregistered_counts_zero = false, int device = 0);
    ~DeviceKmerCounter() override;
    DeviceKmerCounter(const DeviceKmerCounter&) = delete;
    DeviceKmerCounter& operator=(const DeviceKmerCounter&) = delete;
    void add_target(std::string_view kmer);
    size_t add_targets_from_table(const std::string& kmers_tsv_gz);
    size_t add_targets_from_sequences(const std::string& fasta);
    void add_targets_of(std::string_view sequence);
    /** `threads` is accepted for the interface's sake: one reader feeds the device */
    void count(const std::string& readfile, unsigned threads = 1);
    size_t getKmerAbundance(std::string kmer) override;
    size_t targets();
    std::vector<size_t> abundance_histogram(size_t max_count);
    size_t kmers_seen();
    /** zero counts and windows seen, keep the registered k-mers: the next sample over the same index */
    void reset_counts();
    /** the C handle (pg_kmer_counter*), for callers that go on with pg_kmer_counter_lookup */
    void* handle() const { return handle_; }

private:
    friend class DeviceCountPlan;
    bool encode_canonical(const char* s, uint64_t& code) const;
    void flush_codes();
    void fetch_table();
    void check(int rc, const char* what) const;
    static constexpr uint64_t kEmpty = ~0ull;
    size_t k_;
    bool lenient_;
    void* handle_ = nullptr;
    bool counting_ = false;               // the first count is behind us: no more targets
    std::vector<uint64_t> codes_;         // add_target's codes, sent in blocks
    std::vector<uint64_t> table_;         // host copy: key, count of slot i at [2i], [2i+1]
    uint64_t cap_ = 0;
    std::atomic<bool> fetched_{false};
    std::mutex fetch_lock_;
};

/** The index-level half of fill_read_kmercounts_all, resident on the device (include/pangenie_counts.h):
 *  every `<prefix>_<chromosome>_kmers.tsv.gz` of the index is read ONCE, its k-mers coded and resolved against the
 *  counter's table; a sample's numbers are then formed by one kernel per sample, without the host copy of the table.
 *  The counter must outlive the plan; both are used from one thread. */
class DeviceCountPlan {
public:
    /** Reads the tables with the checks of fill_read_kmercounts (foreign chromosome, more lines than variants, position
     *  mismatch) and two of its own (fewer lines than variants; the unique k-mers of a line are not UniqueKmers::size()).
     *  `register_targets`: also registers every k-mer of the tables with the counter (in place of a separate
     *  add_targets_from_table pass; the counter must not have counted yet).  A k-mer that is not registered: throws unless
     *  the counter was made with unregistered_counts_zero. */
    DeviceCountPlan(DeviceKmerCounter& counter, UniqueKmersMap& index, const std::string& prefix, bool register_targets);
    ~DeviceCountPlan();
    DeviceCountPlan(const DeviceCountPlan&) = delete;
    DeviceCountPlan& operator=(const DeviceCountPlan&) = delete;
    /** the numbers fill_read_kmercounts_all + SampleCounts::of give for the reads counted so far */
    SampleCounts fill(size_t kmer_coverage);
    /** the same numbers into arrays in the memory of the counter's device, one pointer per chromosome in chromosomes()
     *  order (a pg_sampler_counts row, include/pangenie_sampler.h: pg_sampler_counts_rows); nothing comes back to the host */
    void fill_device(size_t kmer_coverage, uint16_t* const* d_kmer_count, uint16_t* const* d_coverage);
    /** update_readcount / set_coverage on every object of `index` (the one the plan was made over, or a copy of it): the
     *  drop-in for fill_read_kmercounts_all */
    void fill_into(UniqueKmersMap* index, size_t kmer_coverage);
    /** straight into sample `sample` of a cohort job over the same index (pg_cohort_new; chromosomes in map order) */
    void fill_job(pg_job* job, uint32_t sample, size_t kmer_coverage);
    /** the C handle (pg_count_plan*) */
    void* handle() const { return handle_; }
    const std::vector<std::string>& chromosomes() const { return names_; }
    size_t unique_kmers() const;
    size_t flanking_kmers() const;
    /** device time of the last fill's kernel, ms */
    double last_fill_ms() const;

private:
    void* handle_ = nullptr;
    std::vector<std::string> names_;
    std::vector<size_t> n_kmers_, n_variants_;   // per chromosome
};

/** genotype_cohort with the counting in it: one DeviceKmerCounter and one DeviceCountPlan over `index` (tables at
 *  `<prefix>_<chromosome>_kmers.tsv.gz`, their k-mers are the registered set), one cohort job for up to `batch` samples; per
 *  sample reset_counts, count(readfiles[s]), fill_job with kmer_coverages[s]; per batch one run.  Returns what
 *  genotype_cohort returns for the SampleCounts of the same samples.  The objects of `index` are not touched. */
std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort_reads(
    UniqueKmersMap& index, const std::string& prefix, const std::vector<std::string>& readfiles, const std::vector<size_t>& kmer_coverages,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    size_t batch = 64);

/** genotype_cohort_sampled with the counting in it — reads -> counts -> sampler -> HMM with only the reads going up: one
 *  DeviceKmerCounter and one DeviceCountPlan over `index` (as genotype_cohort_reads makes them); per batch of up to `batch`
 *  samples one pg_sampler_counts; per sample reset_counts, count(readfiles[s]), fill_device into that sample's rows; per batch
 *  pg_sampler_cohort_new_device (the counts are read where they lie), one run, and the fetch: 2 bytes of coverage per variant
 *  and the reduced panels come back.  Returns what genotype_cohort_sampled returns for the SampleCounts of the same samples,
 *  `sampled` (may be null) the same SampledPaths.  The objects of `index` are not touched.  C ABI errors become
 *  std::runtime_error; when a batch does not fit the device (PG_ERR_NOMEM) the message says to lower `batch`: batches are
 *  never split here. */
std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort_sampled_reads(
    UniqueKmersMap& index, const std::string& prefix, const std::vector<std::string>& readfiles, const std::vector<size_t>& kmer_coverages,
    size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    size_t batch = 64, std::vector<std::map<std::string, SampledPaths>>* sampled = nullptr);

/** The whole default pipeline — reads in, VCF sample columns out: genotype_cohort_sampled_reads with the tail
 *  of genotype_cohort_sampled_record_fields behind pg_sampler_cohort_new_device, batch by batch.  The arguments of
 *  genotype_cohort_sampled_reads plus the chromosomes' graphs and `ignore_imputed`; per sample and chromosome the record
 *  fields, the coverage and the reduced panel's unique k-mer count per bubble: what
 *  Graph::genotypes_records(fields, coverage, unique_kmers, ignore_imputed) prints equals the lines of
 *  genotype_cohort_sampled_reads' normalised results.  Refusals as both. */
std::vector<std::map<std::string, SampledRecordFields>> genotype_cohort_sampled_reads_record_fields(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    size_t batch = 64, bool ignore_imputed = false, std::vector<std::map<std::string, SampledPaths>>* sampled = nullptr);

/** The same with the sample column formed as text on the device (pg_job_record_text reads KC from the coverage
 *  the count plan wrote on the device): per sample and chromosome a RecordText, as genotype_cohort_sampled_record_text returns it;
 *  Graph::genotypes_records(text) prints the sibling's lines. */
std::vector<std::map<std::string, RecordText>> genotype_cohort_sampled_reads_record_text(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    size_t batch = 64, bool ignore_imputed = false, std::vector<std::map<std::string, SampledPaths>>* sampled = nullptr);

/** ... and with the lines joined on the device: per sample and chromosome the RecordLines of
 *  genotype_cohort_sampled_record_lines, from reads. */
std::vector<std::map<std::string, RecordLines>> genotype_cohort_sampled_reads_record_lines(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    size_t batch = 64, bool ignore_imputed = false, std::vector<std::map<std::string, SampledPaths>>* sampled = nullptr);

/** sample_cohort_panel_text / _lines (graph_io.hpp) from reads: the batches of genotype_cohort_sampled_reads,
 *  per job the sampled-panel VCF's haplotype columns or whole lines from the device; no job is run. */
std::vector<std::map<std::string, RecordText>> sample_cohort_reads_panel_text(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    size_t batch = 64);
std::vector<std::map<std::string, RecordLines>> sample_cohort_reads_panel_lines(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    size_t batch = 64);

/** The reader of the counters' count() on its own: the sequences of a FASTA / FASTQ file (plain or gzipped) in batches of
 *  about `batch_bytes`, back to back with a newline after each, handed to `sink`; returns the bytes of all batches.  With a sink
 *  that drops its batch this is the ceiling of any design with one host reader (tools/bench_kmer_counter.py). */
size_t for_each_read_batch(const std::string& readfile, const std::function<void(std::string_view)>& sink, size_t batch_bytes = (size_t)4 << 20);

/** one row of `<prefix>_<chromosome>_kmers.tsv(.gz)` — the reference's interface (src/kmerparser.hpp); implemented
 *  over an in-place column scanner (kmer_counts.cpp: KmerRow) */
void parse_kmer_line(std::string line, std::string& chrom, size_t& start, std::vector<std::string>& kmers,
                     std::vector<std::string>& flanking_kmers, bool& is_header);

/** local coverage of a variant = integer mean of the flanking k-mers' read counts inside [coverage / 4, coverage * 4],
 *  the given coverage when none qualifies (behaviour: src/kmerparser.cpp:32-53) */
unsigned short compute_local_coverage(std::vector<std::string>& kmers, KmerCounter& read_counts, size_t kmer_coverage);

/** The count-filling part of the reference's fill_read_kmercounts (src/commands.cpp:74-139): for every variant of
 *  `chromosome`, update_readcount(i, count of the i-th unique k-mer) and set_coverage(local coverage), reading the
 *  k-mers from the gzipped table PanGenie-index wrote.  (The reference's function goes on to run the HaplotypeSampler:
 *  that is pangenie::HaplotypeSampler, on the GPU.)  Throws std::runtime_error where the reference asserts. */
void fill_read_kmercounts(const std::string& chromosome, UniqueKmersMap* unique_kmers_map, KmerCounter& read_kmer_counts,
                          const std::string& kmers_tsv_gz, size_t kmer_coverage);

/** fill_read_kmercounts for every chromosome of the index, `threads` chromosomes at a time (the reference's thread pool
 *  around it, src/commands.cpp:857-868), tables at `<prefix>_<chromosome>_kmers.tsv.gz`.  The counter is only read; the
 *  first exception of a worker is rethrown after all have stopped. */
void fill_read_kmercounts_all(UniqueKmersMap* unique_kmers_map, KmerCounter& read_kmer_counts, const std::string& prefix,
                              size_t kmer_coverage, unsigned threads = 1);

}  // namespace pangenie
