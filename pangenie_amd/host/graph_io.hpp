// graph_io.hpp — the consumer side of the path: the `<prefix>_<chromosome>_Graph.cereal` archive PanGenie-index writes
// (reference Graph::save, src/graph.hpp:79-87) read WITHOUT cereal, the un-merging of combined variant bubbles
// (behaviour: Variant::separate_variants, src/variant.cpp:308-383) and the text of a genotyped VCF (behaviour:
// Graph::write_genotypes, src/graph.cpp:118-278) — SURVEY.md §8(f)-4.  Host code; the likelihoods it prints come from
// the device (pangenie::HMM).
//
// Archive layout (cereal binary: little endian, no framing; member order of the reference's serialize functions):
//   Graph    = FastaReader · chromosome string · kmer_size u64 · add_reference u8 · variants_deleted u8 ·
//              vector<shared_ptr<Variant>> · variant_ids vector<vector<string>>                  (src/graph.hpp:79-87)
//   FastaReader = map<string, shared_ptr<DnaSequence>>                                           (src/fastareader.hpp:40-43)
//   DnaSequence = vector<u8> (two bases per byte, first base in the high nibble: A C G T = 0 1 2 3, anything else 4) ·
//              even_length u8 · is_undefined u8                                                  (src/dnasequence.hpp:48-51)
//   Variant  = left_flank · right_flank · inner_flanks vector<DnaSequence> · chromosome · start_position u64 ·
//              allele_sequences vector<vector<DnaSequence>> (one list per merged VCF record) · allele_combinations
//              vector<vector<u16>> (bubble allele -> allele of each record) · uncovered_alleles vector<vector<u16>> ·
//              paths vector<u16> (bubble allele of every panel path) · flanks_added u8          (src/variant.hpp:93-96)
//   shared_ptr<T> (T not polymorphic) = id u32, MSB set the first time the object occurs (its data follows), 0 = null;
//              ids count up from 1 over ALL shared pointers of the archive
//   string = u64 length + bytes · vector<T> = u64 n + elements (arithmetic T: raw)
// Checked byte for byte on the reference's fixture tests/data/index_chr1_Graph.cereal (kept as data under tests/golden/).
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "pangenie_host.hpp"

namespace pangenie {

/** A DNA string in the archive's packed form. */
class DnaSequence {
public:
    DnaSequence() = default;
    explicit DnaSequence(const std::string& bases);
    size_t size() const { return packed_.size() * 2 - (even_length_ ? 0 : 1); }
    char operator[](size_t position) const;
    std::string to_string() const;
    void append(const DnaSequence& other);
    /** the archive's flag (set when a base outside ACGT was appended; not recomputed from the content) */
    bool contains_undefined() const { return undefined_; }
    bool operator==(const DnaSequence& o) const { return packed_ == o.packed_ && even_length_ == o.even_length_; }
    // archive form
    const std::vector<unsigned char>& packed() const { return packed_; }
    bool even_length() const { return even_length_; }
    static DnaSequence from_archive(std::vector<unsigned char> packed, bool even_length, bool undefined);

private:
    std::vector<unsigned char> packed_;
    bool even_length_ = true, undefined_ = false;
};

/** One record of the output VCF: a (single, un-merged) variant with its alleles, what the panel paths carry and the
 *  genotype likelihoods that belong to it. */
struct VcfSite {
    std::string chromosome;
    size_t start = 0;                         // 0-based
    std::vector<std::string> alleles;         // [0] = REF
    std::vector<bool> undefined;              // allele contains a base outside ACGT
    std::vector<unsigned short> paths;        // allele of every panel path
    GenotypingResult likelihoods;             // over this record's alleles
    std::vector<unsigned short> sampled;      // allele of every sampled haplotype (records() with a sampled panel)
};

/** what the HaplotypeSampler left of a bubble: the bubble allele of every sampled haplotype and the number of unique k-mers
 *  still counted (reference src/sampledpanel.hpp; filled from UniqueKmers::get_path_ids + size(), src/commands.cpp:994-1005) */
struct SampledPanel {
    std::vector<unsigned short> path_to_allele;
    size_t unique_kmers = 0;
};

/** What the bubbles of a graph mean for their single VCF records, flat: the C ABI's pg_record_plan (include/pangenie_hmm.h,
 *  DESIGN.md 4e "Records").  Bubble v owns the records rec_off[v] .. rec_off[v + 1] - 1 (graph order: the order of
 *  Graph::genotypes_records); per record r: map[map_off[r] + id] = the record allele that bubble allele id carries
 *  (Variant's allele_combinations[id][r]), n_alleles[r], and for every record allele its index among the record's defined
 *  alleles (vcf_index[vcf_off[r] + a]; 0xFFFF: the allele's sequence is undefined). */
struct RecordPlan {
    std::vector<uint32_t> rec_off, map_off, vcf_off;
    std::vector<uint16_t> map, n_alleles, vcf_index;
    size_t nr_of_records() const { return n_alleles.size(); }
    /** the C view; valid as long as this object is */
    pg_record_plan view() const;
};

/** The sample column of a chromosome's VCF lines as the device forms it, per single record in
 *  Graph::genotypes_records order: `calls` the GT and GQ (genotype_cohort_record_calls), `gl` the GL values — record r's at
 *  gl_off[r] .. gl_off[r + 1] - 1, genotype (a <= b) over its defined alleles at b (b + 1) / 2 + a (C ABI pg_job_record_gl).
 *  As genotype_cohort_record_fields returns it, no entry is deferred any more. */
struct RecordFields {
    std::vector<GenotypeCall> calls;
    std::vector<pg_gl> gl;
    std::vector<uint64_t> gl_off;
};

/** The sample column of a chromosome's VCF lines as BYTES (DESIGN.md 4e-6, C ABI pg_job_record_text): record r's
 *  `GT:GQ:GL:KC` is bytes[off[r] .. off[r + 1]), records in Graph::genotypes_records order, and `unique_kmers` — one entry per
 *  bubble — is what the INFO column needs of the sample (UK).  As genotype_cohort_record_text returns it, no record is empty
 *  except one of fewer than three GL values, which Graph::genotypes_records refuses as it does everywhere. */
struct RecordText {
    std::vector<uint64_t> off;
    std::string bytes;
    std::vector<unsigned short> unique_kmers;
};

/** Whole VCF lines of a chromosome as BYTES (DESIGN.md 4e-7, C ABI pg_job_record_lines): line r — the fixed columns, one
 *  `GT:GQ:GL:KC` column per sample behind a tab each, a newline — is bytes[off[r] .. off[r + 1]), records in
 *  Graph::genotypes_records order.  As genotype_cohort_record_lines returns it no line is empty. */
struct RecordLines {
    std::vector<uint64_t> off;
    std::string bytes;
};

/** The lines of a chromosome with those the device left to the host (length 0 in `device`) composed here: prefix[r], then
 *  per sample a tab and its FINISHED text of the record (genotype_cohort_record_text's), a newline.  Every other line is
 *  copied as it is.  Throws where a sample's text of such a record is empty too (fewer than three likelihoods), and on
 *  arrays that do not fit each other. */
RecordLines compose_record_lines(const std::vector<std::string>& prefix, const std::vector<const RecordText*>& texts, const RecordLines& device);

/** `GT:GQ:GL:KC` of record q from finished record fields: what Graph::genotypes_records(fields, ...) prints of it (the rule
 *  the device's text follows).  Throws on fewer than three values and on a value that is still deferred. */
std::string record_field_text(const RecordFields& fields, size_t q, unsigned short coverage, bool no_call);

/** A variant bubble of the graph: one or several VCF records closer than the k-mer size, merged
 *  (reference src/variant.hpp:28-121). */
class Variant {
public:
    Variant() = default;
    /** a bubble from its stored parts (what the archive holds; see the layout above): `records` = the allele strings of
     *  every merged VCF record, `between` = the reference sequence between neighbouring records, `combinations` = for
     *  every bubble allele the allele of each record, `paths` = bubble allele of every panel path */
    static Variant from_parts(const std::string& chromosome, size_t start_position, const std::string& left_flank, const std::string& right_flank,
                              const std::vector<std::vector<std::string>>& records, const std::vector<std::string>& between,
                              const std::vector<std::vector<unsigned short>>& combinations, const std::vector<unsigned short>& paths,
                              bool flanks_added);
    size_t nr_of_alleles() const { return allele_combinations_.size(); }
    size_t nr_of_paths() const { return paths_.size(); }
    size_t nr_of_records() const { return allele_sequences_.size(); }
    bool is_combined() const { return allele_sequences_.size() > 1; }
    size_t get_start_position() const { return start_position_; }
    size_t get_end_position() const;
    const std::string& get_chromosome() const { return chromosome_; }
    unsigned short get_allele_on_path(size_t path) const { return paths_.at(path); }
    /** sequence of bubble allele `index`: the records' alleles joined by the reference between them, with the flanks
     *  when the bubble carries them */
    std::string get_allele_string(size_t index) const;
    bool is_undefined_allele(size_t index) const;
    /** the bubble as its single records (positions, alleles, path alleles), and `result` — likelihoods over bubble
     *  alleles — folded onto each record's own alleles (genotypes that agree on a record's alleles add up);
     *  coverage / unique k-mer count are the bubble's.  `result` may be null. */
    std::vector<VcfSite> records(const GenotypingResult* result, const SampledPanel* sampled = nullptr) const;

private:
    friend class Graph;
    DnaSequence left_flank_, right_flank_;
    std::vector<DnaSequence> inner_flanks_;
    std::string chromosome_;
    size_t start_position_ = 0;
    std::vector<std::vector<DnaSequence>> allele_sequences_;
    std::vector<std::vector<unsigned short>> allele_combinations_, uncovered_alleles_;
    std::vector<unsigned short> paths_;
    bool flanks_added_ = false;
};

class Graph {
public:
    Graph() = default;
    /** throw std::runtime_error on malformed input */
    static Graph parse(const std::vector<unsigned char>& bytes);
    static Graph load(const std::string& path);
    std::vector<unsigned char> serialize() const;
    /** a graph from bubbles that exist already (tests; hosts that build their bubbles elsewhere): `variant_ids` = one row
     *  per single VCF record in graph order, the ids of its ALT alleles in the lexicographic order of the allele sequences
     *  (what the archive stores), or empty */
    static Graph from_parts(const std::string& chromosome, size_t kmer_size, bool reference_added, const std::vector<Variant>& variants,
                            const std::vector<std::vector<std::string>>& variant_ids);
    /** the same with the chromosome's reference sequence (what PanGenie-index keeps in the graph: index_builder.hpp) */
    static Graph from_parts(const std::string& chromosome, size_t kmer_size, bool reference_added, const std::vector<Variant>& variants,
                            const std::vector<std::vector<std::string>>& variant_ids, const std::string& reference_bases);

    size_t get_kmer_size() const { return kmer_size_; }
    const std::string& get_chromosome() const { return chromosome_; }
    bool reference_added() const { return add_reference_; }
    size_t size() const { return variants_.size(); }
    const Variant& get_variant(size_t index) const;
    const std::vector<std::vector<std::string>>& variant_ids() const { return variant_ids_; }
    /** reference sequence the graph was built on */
    std::string reference(const std::string& name) const;
    /** the record plan of this graph's bubbles (depends on the index alone: one per chromosome, shared by all samples) */
    RecordPlan record_plan() const;

    /** the header lines of a genotyped VCF (reference src/graph.cpp:137-149); `date` = yyyymmdd, today when empty */
    static std::vector<std::string> genotypes_header(const std::string& sample, const std::string& date = "");
    /** ... with one column per sample: the names joined by tabs */
    static std::vector<std::string> genotypes_header(const std::vector<std::string>& samples, const std::string& date = "");
    /** per record, in genotypes_records order, what a genotyped line holds in front of the sample columns:
     *  `CHROM .. INFO\tGT:GQ:GL:KC` without a trailing tab (UK from `unique_kmers`, one entry per bubble).  It depends on the
     *  index alone: one array per chromosome, whatever the number of samples (the prefix of pg_job_line_prefix). */
    std::vector<std::string> genotypes_fixed_columns(const std::vector<unsigned short>& unique_kmers) const;
    /** the same columns with the digits of UK left out, and per record where they belong: slot[r] = the position behind
     *  `;UK=`.  genotypes_fixed_columns(uk)[r] is this record's string with the decimal uk of its bubble put in at slot[r].
     *  It depends on the graph alone: one array per chromosome of a SAMPLED cohort, whose chains differ in UK only (the
     *  slotted prefix of pg_job_line_prefix_strided). */
    std::vector<std::string> genotypes_fixed_columns_slotted(std::vector<uint32_t>* slot) const;
    /** the record lines: one per single variant, in graph order; `genotyping_result` = one (normalised) result per
     *  bubble, as HMM::get_genotyping_result() returns them */
    std::vector<std::string> genotypes_records(const std::vector<GenotypingResult>& genotyping_result, bool ignore_imputed = false) const;
    /** header (when asked for) + records into `filename` (appending without header), like the reference's
     *  Graph::write_genotypes */
    void write_genotypes(const std::string& filename, const std::vector<GenotypingResult>& genotyping_result, bool write_header,
                         const std::string& sample, bool ignore_imputed = false) const;

    /** the same lines from the device's record fields, without a likelihood on the host: the fixed columns as above (UK from
     *  `unique_kmers`, one entry per bubble), GT and GQ from the calls (`.` for a bubble without unique k-mers under
     *  `ignore_imputed`), GL from pg_gl_text, KC from `coverage` (one entry per bubble: the sample's local coverage) */
    std::vector<std::string> genotypes_records(const RecordFields& fields, const std::vector<unsigned short>& coverage,
                                               const std::vector<unsigned short>& unique_kmers, bool ignore_imputed = false) const;
    void write_genotypes(const std::string& filename, const RecordFields& fields, const std::vector<unsigned short>& coverage,
                         const std::vector<unsigned short>& unique_kmers, bool write_header, const std::string& sample, bool ignore_imputed = false) const;

    /** the same lines with the sample column arriving as bytes: the fixed columns as above (UK from text.unique_kmers), the
     *  column spliced in.  Throws where a record's text is empty: fewer than three likelihoods, or a record nobody finished. */
    std::vector<std::string> genotypes_records(const RecordText& text) const;
    void write_genotypes(const std::string& filename, const RecordText& text, bool write_header, const std::string& sample) const;
    /** a multi-sample VCF: the header (when asked for) with the samples' names, then the lines' bytes in ONE write.  Throws on
     *  offsets that do not fit the bytes or the graph's records, and on an empty line. */
    void write_genotypes(const std::string& filename, const RecordLines& lines, bool write_header, const std::vector<std::string>& samples) const;

    /** the phasing VCF of a `-p` run (reference Graph::write_phasing, src/graph.cpp:280-412): the same fixed columns, `GT:KC`
     *  with the Viterbi haplotypes `a|b` (HMM with run_phasing; `.` for an allele of undefined sequence) */
    static std::vector<std::string> phasing_header(const std::string& sample, const std::string& date = "");
    /** ... with one column per sample: the names joined by tabs */
    static std::vector<std::string> phasing_header(const std::vector<std::string>& samples, const std::string& date = "");
    std::vector<std::string> phasing_records(const std::vector<GenotypingResult>& genotyping_result, bool ignore_imputed = false) const;
    void write_phasing(const std::string& filename, const std::vector<GenotypingResult>& genotyping_result, bool write_header,
                       const std::string& sample, bool ignore_imputed = false) const;
    /** per record, in phasing_records order, what a phased line holds in front of the sample columns: `CHROM .. INFO\tGT:KC`
     *  without a trailing tab (UK from `unique_kmers`, one entry per bubble): the prefix of pg_job_phased_line_prefix */
    std::vector<std::string> phasing_fixed_columns(const std::vector<unsigned short>& unique_kmers) const;
    /** the phased lines with the `GT:KC` column arriving as bytes (DESIGN.md 4e-9, C ABI pg_job_phased_text): the fixed
     *  columns as above (UK from text.unique_kmers), the column spliced in.  Throws where a record's text is empty. */
    std::vector<std::string> phasing_records(const RecordText& text) const;
    /** a multi-sample phasing VCF: the header (when asked for) with the samples' names, then the lines' bytes in ONE write.
     *  Throws on offsets that do not fit the bytes or the graph's records, and on an empty line. */
    void write_phasing(const std::string& filename, const RecordLines& lines, bool write_header, const std::vector<std::string>& samples) const;
    /** a record whose REF holds a base outside ACGT: the record plan calls REF defined whatever it holds, the host prints `.`
     *  for a haplotype on it — the device's phasing column is not the host's for such a graph (phase_cohort_record_text) */
    bool has_undefined_reference_allele() const;

    /** the sampled panel as a VCF (`-d`; reference Graph::write_sampled_panel, src/graph.cpp:414-547): one column per sampled
     *  haplotype (`sampledHT<i>`), its allele among the record's defined ones, `.` where it carries undefined sequence */
    static std::vector<std::string> sampled_panel_header(size_t nr_paths, const std::string& date = "");
    std::vector<std::string> sampled_panel_records(const std::vector<SampledPanel>& sampled_paths) const;
    void write_sampled_panel(const std::string& filename, const std::vector<SampledPanel>& sampled_paths, bool write_header) const;
    /** per record, in sampled_panel_records order, what a panel line holds in front of the haplotype columns:
     *  `CHROM .. INFO\tGT` without a trailing tab (UK from `unique_kmers`, one entry per bubble: SampledPanel::unique_kmers) */
    std::vector<std::string> sampled_panel_fixed_columns(const std::vector<unsigned short>& unique_kmers) const;
    /** the same columns with the digits of UK left out and slot[r] = where they belong, as genotypes_fixed_columns_slotted:
     *  the slotted prefix of pg_job_panel_line_prefix_strided */
    std::vector<std::string> sampled_panel_fixed_columns_slotted(std::vector<uint32_t>* slot) const;
    /** the panel lines with the haplotype columns arriving as bytes (C ABI pg_job_panel_text): the fixed columns as above
     *  (UK from text.unique_kmers), the columns spliced in.  Throws where a record's text is empty. */
    std::vector<std::string> sampled_panel_records_of_text(const RecordText& text) const;
    /** (the same under the siblings' name; a template, so that a braced list still means the SampledPanels) */
    template <class Text, class = typename std::enable_if<std::is_same<Text, RecordText>::value>::type>
    std::vector<std::string> sampled_panel_records(const Text& text) const { return sampled_panel_records_of_text(text); }
    /** header (when asked for) for `nr_paths` haplotype columns, then the lines' bytes in ONE write.  Throws on offsets that
     *  do not fit the bytes or the graph's records, and on an empty line. */
    void write_sampled_panel(const std::string& filename, const RecordLines& lines, bool write_header, size_t nr_paths) const;

private:
    struct DeviceFields {   // the sample column from the device's record fields instead of a GenotypingResult per bubble
        const RecordFields* fields;
        const std::vector<unsigned short>* coverage;
        const std::vector<unsigned short>* unique_kmers;
        const RecordText* text = nullptr;   // the column as bytes: fields and coverage are not looked at
        bool panel = false;                 // ... the haplotype columns of the sampled panel (FORMAT `GT`)
    };
    std::vector<std::string> sample_records(const std::vector<GenotypingResult>& genotyping_result, bool ignore_imputed, bool phasing,
                                            const std::vector<SampledPanel>* sampled_paths = nullptr, const DeviceFields* device = nullptr) const;
    /** CHROM .. INFO and `format` of every record: genotypes_fixed_columns and phasing_fixed_columns */
    std::vector<std::string> fixed_columns(const std::vector<unsigned short>& unique_kmers, const char* who, const char* format) const;
    /** the slotted columns of genotypes_fixed_columns_slotted and sampled_panel_fixed_columns_slotted (`method`: the caller, as a refusal names it) */
    std::vector<std::string> fixed_columns_slotted(std::vector<uint32_t>* slot, const char* who, const char* method, const char* format) const;
    /** header lines (when asked for), then the lines' bytes in one write: the writers of whole lines */
    enum class LinesOf { Genotypes, Phasing, SampledPanel };
    void write_lines(const std::string& filename, const RecordLines& lines, const std::vector<std::string>* header, LinesOf of) const;
    /** CHROM .. INFO of one record (the ONE place that forms them): `defined` comes back as the record's defined alleles.
     *  With `uk_slot` the digits of `unique_kmers` are left out and *uk_slot = where they belong. */
    std::string fixed_columns_of(const VcfSite& site, size_t record_index, size_t unique_kmers, const char* who, std::vector<unsigned short>& defined,
                                 size_t* uk_slot = nullptr) const;
    size_t nr_of_records() const;
    std::vector<std::pair<std::string, std::shared_ptr<DnaSequence>>> fasta_;   // name -> sequence, archive (= sorted) order
    std::string chromosome_;
    size_t kmer_size_ = 0;
    bool add_reference_ = false, variants_deleted_ = false;
    std::vector<std::shared_ptr<Variant>> variants_;
    std::vector<std::vector<std::string>> variant_ids_;
};

/** genotype_cohort_calls per VCF RECORD: the arguments of genotype_cohort_calls plus the chromosomes' graphs.  Per sample and
 *  chromosome one GenotypeCall per single record, in Graph::genotypes_records order, holding what the GT and GQ columns of
 *  that line say: allele_1 / allele_2 are indices among the record's DEFINED alleles, -1 / -1 and quality 0 for `.`.  The
 *  records are formed on the device (C ABI pg_job_record_plan / pg_job_record_calls; one plan per chromosome, uploaded once);
 *  the records of a bubble the device deferred are formed here from that bubble's bins through Variant::records and
 *  genotype_field's rules.  `ignore_imputed`: a bubble without unique k-mers gives no call. */
std::vector<std::map<std::string, std::vector<GenotypeCall>>> genotype_cohort_record_calls(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false,
    long double effective_N = 25000.0L, int device = 0, bool ignore_imputed = false);

/** The whole sample column per VCF RECORD from one job: the arguments and the calls of genotype_cohort_record_calls, and the
 *  GL values of every record (C ABI pg_job_record_gl) — no genotype bin leaves the device.  Entries the device deferred (a
 *  bubble next to long double's subnormals; a value whose fourth digit the fp64 logarithm could not vouch for, about 2e-9 of
 *  them) are finished here from that bubble's bins through Variant::records and genotype_field's rules.  Per sample and
 *  chromosome what Graph::genotypes_records(fields, coverage, unique_kmers) prints. */
std::vector<std::map<std::string, RecordFields>> genotype_cohort_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false,
    long double effective_N = 25000.0L, int device = 0, bool ignore_imputed = false);

/** The sample column of one chromosome of a SAMPLED cohort: the record fields, and per bubble what the other columns of the
 *  line need of the sample — the local coverage (KC) and the unique k-mer count of the sample's reduced panel (UK; 0 for
 *  every bubble of a chain without a kept column).  Graph::genotypes_records(fields, coverage, unique_kmers, ignore_imputed)
 *  prints the lines. */
struct SampledRecordFields {
    RecordFields fields;
    std::vector<unsigned short> coverage, unique_kmers;
};

/** genotype_cohort_sampled for a caller who wants VCF lines: the arguments of genotype_cohort_sampled plus the
 *  chromosomes' graphs and `ignore_imputed`.  pg_sampler_cohort_new, one pg_job_record_plan_strided per chromosome (the plan is
 *  checked and uploaded once for all samples), the run, pg_job_record_calls, pg_job_record_gl and the two packed fetches: no
 *  reduced panel and no genotype bin comes back, except for a chain with an entry the device deferred, which is finished from
 *  that chain's own reduced panel and bins as genotype_cohort_record_fields finishes them.  The lines equal those of
 *  Graph::genotypes_records on genotype_cohort_sampled's normalised results.  `sampled` as in genotype_cohort_sampled.  Throws
 *  std::runtime_error on a missing graph, a graph whose bubble count is not the index's, samples that do not fit, and on the C
 *  ABI's errors. */
std::vector<std::map<std::string, SampledRecordFields>> genotype_cohort_sampled_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    bool ignore_imputed = false, std::vector<std::map<std::string, SampledPaths>>* sampled = nullptr);

/** genotype_cohort_record_fields with the sample column formed as TEXT on the device: the same job, then
 *  pg_job_record_text and ONE packed fetch of the bytes and their offsets; neither calls nor GL values come back, except for a
 *  chain with a record the device left to the host (a deferred call or GL value), whose fields are fetched, finished as
 *  genotype_cohort_record_fields finishes them and printed by record_field_text.  Graph::genotypes_records(text) gives the
 *  lines of Graph::genotypes_records(fields, coverage, unique_kmers, ignore_imputed) on the sibling's output. */
std::vector<std::map<std::string, RecordText>> genotype_cohort_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false,
    long double effective_N = 25000.0L, int device = 0, bool ignore_imputed = false);

/** genotype_cohort_record_text with the LINES joined on the device too: the same job and the record text,
 *  one pg_job_line_prefix per chromosome (Graph::genotypes_fixed_columns: formed and uploaded once, whatever the number of
 *  samples), pg_job_record_lines and ONE packed fetch.  Per chromosome the multi-sample lines, sample s in column 9 + s; a
 *  line the device left to the host is composed here from the prefix and the finished texts (compose_record_lines), so no
 *  line is empty; a record of fewer than three values throws.  Throws if the samples' unique k-mer counts of a chromosome
 *  differ: a multi-sample line has one INFO column (over a shared index they cannot).  Sampled cohorts, whose UK and reduced
 *  panels differ per sample, have genotype_cohort_sampled_record_lines.  Not covered: the combined (-a) records (the phasing
 *  column has phase_cohort_record_lines). */
std::map<std::string, RecordLines> genotype_cohort_record_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false,
    long double effective_N = 25000.0L, int device = 0, bool ignore_imputed = false);

/** genotype_cohort_sampled_record_fields with the sample column formed as text on the device, as genotype_cohort_record_text. */
std::vector<std::map<std::string, RecordText>> genotype_cohort_sampled_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    bool ignore_imputed = false, std::vector<std::map<std::string, SampledPaths>>* sampled = nullptr);

/** genotype_cohort_sampled_record_text with the LINES joined on the device too: the same job, the strided plans,
 *  the run and pg_job_record_text, then ONE slotted prefix per chromosome (Graph::genotypes_fixed_columns_slotted through
 *  pg_job_line_prefix_strided: the device prints every chain's own UK at the slot), pg_job_record_lines and ONE packed fetch.
 *  Per sample and chromosome the single-sample lines — the '\n'-joined Graph::genotypes_records of the sibling's text —, which
 *  Graph::write_genotypes(filename, lines, ...) writes.  Neither text nor k-mer counts come back, except for a chain with a line
 *  the device left to the host: that chain's counts and text are fetched, the text finished as the sibling finishes it, and the
 *  lines composed over a prefix formed with that chain's UK (compose_record_lines).  A record of fewer than three values
 *  throws.  Not covered: the combined (-a) records; the phasing column over slotted prefixes. */
std::vector<std::map<std::string, RecordLines>> genotype_cohort_sampled_record_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0,
    bool ignore_imputed = false, std::vector<std::map<std::string, SampledPaths>>* sampled = nullptr);

/** The SAMPLED-PANEL VCF of a sampled cohort from the device (the `-d` output, all that PanGenie-sampling
 *  writes): pg_sampler_cohort_new with sampled_paths = NULL, one strided plan per chromosome, pg_job_panel_text — no run —,
 *  and ONE packed fetch of the bytes and their offsets (one more of the records' UK): no reduced panel and no pick comes
 *  back.  Per sample and chromosome the haplotype columns of every record and, per bubble, the panel's own unique k-mer
 *  count; Graph::sampled_panel_records(text) gives the lines of Graph::sampled_panel_records over the SampledPanels of
 *  genotype_cohort_sampled(..., &sampled).  A chromosome with a record whose REF is of undefined sequence
 *  (Graph::has_undefined_reference_allele: the plan calls REF defined, the host prints `.` for a haplotype on it) and a
 *  panel of more than 64 paths go down the host route — pg_job_fetch_panel per chain, SampledPanels,
 *  Graph::sampled_panel_records.  Throws as genotype_cohort_sampled_record_text does. */
std::vector<std::map<std::string, RecordText>> sample_cohort_panel_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0);

/** ... with the LINES joined on the device too: ONE slotted prefix per chromosome (Graph::sampled_panel_fixed_columns_slotted
 *  through pg_job_panel_line_prefix_strided: the device prints every chain's own UK at the slot), pg_job_panel_lines and ONE
 *  packed fetch, of the lines alone.  Per sample and chromosome the lines — the '\n'-joined Graph::sampled_panel_records —,
 *  which Graph::write_sampled_panel(filename, lines, ...) writes. */
std::vector<std::map<std::string, RecordLines>> sample_cohort_panel_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false, long double effective_N = 25000.0L, int device = 0);

/** The phasing job of a `-p` run to VCF text (reference src/commands.cpp:936-966, Graph::write_phasing): a
 *  phasing-only cohort job over `only_paths` (null: all paths; the Viterbi kernels take at most 64, the reference passes at
 *  most 30) with the setup of the genotype_cohort_record_* drivers — one plan per chromosome, whatever the number of samples —,
 *  the run, pg_job_phased_text and ONE packed fetch of the bytes and their offsets: no haplotype comes back.  Per sample and
 *  chromosome the `GT:KC` column of every record and, per bubble, UK as pg_job_fetch reports it (set at the COLUMN index);
 *  Graph::phasing_records(text) gives the lines of Graph::phasing_records(results, ignore_imputed) on an HMM(..., false, true,
 *  ...)'s results.  Every graph is checked once: a chromosome with a record whose REF is of undefined sequence
 *  (Graph::has_undefined_reference_allele) gets no plan and goes down the host route — pg_job_fetch's haplotypes, one
 *  GenotypingResult per bubble, Graph::phasing_records — inside the same job.  Throws std::runtime_error on a missing graph, a
 *  graph whose bubble count is not the index's, samples that do not fit, and on the C ABI's errors. */
std::vector<std::map<std::string, RecordText>> phase_cohort_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, std::vector<unsigned short>* only_paths = nullptr, double recombrate = 1.26,
    bool uniform = false, long double effective_N = 25000.0L, int device = 0, bool ignore_imputed = false);

/** The multi-sample phasing VCF with the LINES joined on the device: the job of phase_cohort_record_text, pg_job_phased_text —
 *  whose bytes stay on the device —, one pg_job_phased_line_prefix per chromosome (Graph::phasing_fixed_columns; UK from
 *  pg_job_fetch's host-side counts), pg_job_phased_lines and ONE packed fetch, of the lines: neither text nor haplotypes come to
 *  the host.  Per chromosome the lines, sample s in column 9 + s, which Graph::write_phasing(filename, lines, ...) writes.  Only a
 *  chromosome on the host route has its chains fetched, and its lines composed here from the fixed columns and the samples'
 *  columns.  Throws if the samples' unique k-mer counts of a chromosome differ: a multi-sample line has one INFO column (over a
 *  shared index and one path selection they cannot). */
std::map<std::string, RecordLines> phase_cohort_record_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, std::vector<unsigned short>* only_paths = nullptr, double recombrate = 1.26,
    bool uniform = false, long double effective_N = 25000.0L, int device = 0, bool ignore_imputed = false);

/** The `-a` flow to VCF lines: genotype_subsets for a caller who wants the sample column.  One job over every
 *  chromosome and subset, the subsets combined on the device (pg_job_combine), the plan of Graph::record_plan() on the index
 *  contig of each group's first chain, pg_job_combined_record_calls, pg_job_combined_record_gl and the two _all fetches: no
 *  genotype bin comes back, except for a chromosome with an entry the device deferred, which is finished from the chains' own
 *  bins added up on the host, as genotype_cohort_record_fields finishes its entries.  Per chromosome the record fields and the
 *  first chain's coverage and unique k-mer counts: Graph::genotypes_records(fields, coverage, unique_kmers, ignore_imputed)
 *  prints the lines of Graph::genotypes_records(genotype_subsets(..., normalize = true), ignore_imputed).  Throws
 *  std::runtime_error on no subsets, a missing graph, a graph whose bubble count is not the index's, and on the C ABI's errors. */
std::map<std::string, SampledRecordFields> genotype_subsets_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<std::vector<unsigned short>>& subsets, ProbabilityTable* probabilities, double recombrate = 1.26, bool uniform = false,
    long double effective_N = 25000.0L, int device = 0, bool ignore_imputed = false);

}  // namespace pangenie
