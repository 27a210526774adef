// test_sampled_record_fields.cpp — the VCF lines of a SAMPLED cohort from the device's record fields
// (pangenie_amd/host/graph_io.hpp: genotype_cohort_sampled_record_fields; kmer_counts.hpp:
// genotype_cohort_sampled_reads_record_fields) against the lines of the route they spare: genotype_cohort_sampled[_reads],
// GenotypingResult::normalize, Graph::genotypes_records on the results.  Text for text, whole lines, with and without
// ignore_imputed; the sampled paths against those of the existing functions.
//   test_sampled_record_fields gpu <index prefix> <reads of sample 1> <reads of sample 2>
//   test_sampled_record_fields cpu          the refusals that need no job; no device
// <index prefix>: as for tests/cpp/test_record_calls_host.cpp (merged bubbles, alleles of undefined sequence).
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../pangenie_amd/host/cereal_io.hpp"
#include "../../pangenie_amd/host/graph_io.hpp"
#include "../../pangenie_amd/host/kmer_counts.hpp"

using namespace pangenie;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        ++g_checks;                                                                       \
        if (!(cond)) { if (++g_failed <= 20) std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
static void run(const char* name, const std::function<void()>& f) {
    const int before = g_failed;
    try { f(); } catch (const std::exception& e) { ++g_failed; std::printf("  EXCEPTION in %s: %s\n", name, e.what()); }
    std::printf("%s %s\n", g_failed == before ? "ok  " : "FAIL", name);
}
static std::string what_of(const std::function<void()>& f) {
    try { f(); } catch (const std::exception& e) { return e.what(); }
    return "";
}

typedef std::vector<std::map<std::string, std::vector<GenotypingResult>>> CohortResults;
typedef std::vector<std::map<std::string, SampledRecordFields>> CohortFields;
typedef std::vector<std::map<std::string, SampledPaths>> CohortPicks;

static bool same_picks(const CohortPicks& a, const CohortPicks& b) {
    if (a.size() != b.size()) return false;
    for (size_t s = 0; s < a.size(); ++s) {
        if (a[s].size() != b[s].size()) return false;
        for (const auto& kv : a[s]) {
            const auto o = b[s].find(kv.first);
            if (o == b[s].end() || o->second.sampled_paths != kv.second.sampled_paths) return false;
        }
    }
    return true;
}

static void cpu_tests() {
    run("genotype_cohort_sampled[_reads]_record_fields refuse a missing graph and a graph with other bubbles, before any job", [] {
        std::vector<unsigned short> alleles = {0, 1};
        auto bubble = [&](size_t pos) -> std::shared_ptr<UniqueKmers> { return std::make_shared<BiallelicUniqueKmers>(pos, alleles); };
        std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> chromosomes;
        chromosomes["chr2"] = {bubble(99), bubble(199)};
        Variant snp = Variant::from_parts("chr2", 99, "AAAA", "CCCC", {{"C", "G"}}, {}, {{0}, {1}}, {0, 1}, true);
        std::map<std::string, Graph> none, short_one;
        short_one["chr2"] = Graph::from_parts("chr2", 4, false, {snp}, {{"id-G"}});   // one bubble, the index has two
        std::vector<SampleCounts> samples(1);
        ProbabilityTable probs(1, 160, 80, 0.01L);
        const std::string missing = what_of([&] { genotype_cohort_sampled_record_fields(chromosomes, none, samples, 7, true, 10, 25000.0L, &probs); });
        CHECK(missing == "genotype_cohort_sampled_record_fields: no graph of chr2 with the index's bubbles");
        const std::string other = what_of([&] { genotype_cohort_sampled_record_fields(chromosomes, short_one, samples, 7, true, 10, 25000.0L, &probs); });
        CHECK(other == missing);
        UniqueKmersMap index;
        index.kmersize = 31;
        index.unique_kmers = chromosomes;
        const std::vector<std::string> reads = {"no-such-file.fa"};
        const std::string r_missing = what_of([&] { genotype_cohort_sampled_reads_record_fields(index, none, "no-such-prefix", reads, {20}, 7, true, 10, 25000.0L, &probs); });
        CHECK(r_missing == "genotype_cohort_sampled_reads_record_fields: no graph of chr2 with the index's bubbles");
        const std::string r_other = what_of([&] { genotype_cohort_sampled_reads_record_fields(index, short_one, "no-such-prefix", reads, {20}, 7, true, 10, 25000.0L, &probs); });
        CHECK(r_other == r_missing);
        CHECK(what_of([&] { genotype_cohort_sampled_reads_record_fields(index, short_one, "no-such-prefix", reads, {}, 7, true, 10, 25000.0L, &probs); }) ==
              "genotype_cohort_sampled_reads_record_fields: one k-mer coverage per read file");
        // nothing to do: no chromosomes, no samples
        std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> empty;
        CHECK(genotype_cohort_sampled_record_fields(empty, none, samples, 7, true, 10, 25000.0L, &probs).size() == 1);
        CHECK(genotype_cohort_sampled_record_fields(chromosomes, none, {}, 7, true, 10, 25000.0L, &probs).empty());
    });
}

// the lines of `got` through the record-field overload against the lines of `want` (normalised) through the existing one
static void compare_lines(const std::map<std::string, Graph>& graphs, const CohortResults& want, const CohortFields& got, bool ignore_imputed,
                          size_t* compared, size_t* no_call, size_t* values) {
    CHECK(got.size() == want.size());
    for (size_t s = 0; s < want.size() && s < got.size(); ++s) {
        CHECK(got[s].size() == want[s].size());
        for (const auto& kv : want[s]) {
            const Graph& graph = graphs.at(kv.first);
            const std::vector<std::string> lines = graph.genotypes_records(kv.second, ignore_imputed);
            const auto found = got[s].find(kv.first);
            CHECK(found != got[s].end());
            if (found == got[s].end()) continue;
            const SampledRecordFields& f = found->second;
            CHECK(f.coverage.size() == graph.size() && f.unique_kmers.size() == graph.size());
            const std::vector<std::string> ours = graph.genotypes_records(f.fields, f.coverage, f.unique_kmers, ignore_imputed);
            CHECK(ours.size() == lines.size() && f.fields.calls.size() == lines.size() && f.fields.gl_off.size() == lines.size() + 1);
            for (size_t r = 0; r < lines.size() && r < ours.size(); ++r) {
                CHECK(ours[r] == lines[r]);
                if (ours[r] != lines[r] && g_failed <= 20) std::printf("    sample %zu record %zu:\n      %s\n      %s\n", s, r, ours[r].c_str(), lines[r].c_str());
                *compared += 1;
                *no_call += lines[r].find("\t.:.:") != std::string::npos;
            }
            for (const pg_gl& x : f.fields.gl) { *values += 1; CHECK(!(x.mant == 0 && x.exp10 == PG_GL_DEFERRED)); }
        }
    }
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") {
        cpu_tests();
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (argc < 5 || std::string(argv[1]) != "gpu") { std::printf("usage: test_sampled_record_fields gpu <index prefix> <reads 1> <reads 2> | cpu\n"); return 2; }
    const std::string prefix = argv[2];
    const std::vector<std::string> reads = {argv[3], argv[4]};
    const std::vector<size_t> coverage = {20, 17};
    const size_t panel_size = 7;
    // (a UniqueKmersMap copies its objects by pointer: every route loads its own)
    auto fresh = [&] { return load_unique_kmers_map(prefix + "_UniqueKmersMap.cereal"); };
    const UniqueKmersMap index = fresh();
    std::map<std::string, Graph> graphs;
    size_t merged = 0, with_undefined = 0, records = 0;
    for (const auto& kv : index.unique_kmers) {
        graphs[kv.first] = Graph::load(prefix + "_" + kv.first + "_Graph.cereal");
        const Graph& g = graphs[kv.first];
        const RecordPlan plan = g.record_plan();
        for (size_t v = 0; v < g.size(); ++v) merged += g.get_variant(v).nr_of_records() >= 2;
        for (size_t r = 0; r < plan.nr_of_records(); ++r) {
            bool undefined = false;
            for (uint32_t i = plan.vcf_off[r]; i < plan.vcf_off[r + 1]; ++i) undefined = undefined || plan.vcf_index[i] == 0xFFFF;
            with_undefined += undefined;
        }
        records += plan.nr_of_records();
    }
    ProbabilityTable probs(1, 160, 80, 0.01L);

    run("Graph::genotypes_records(genotype_cohort_sampled_record_fields) = Graph::genotypes_records(genotype_cohort_sampled + normalize), two samples", [&] {
        CHECK(merged >= 1);           // the input holds what this test is about
        CHECK(with_undefined >= 1);
        UniqueKmersMap m = fresh(), other = fresh();
        std::vector<SampleCounts> counts;
        {
            DeviceKmerCounter dev(m.kmersize);
            DeviceCountPlan plan(dev, m, prefix, true);
            for (size_t s = 0; s < 2; ++s) {
                dev.reset_counts();
                dev.count(reads[s]);
                counts.push_back(plan.fill(coverage[s]));
            }
        }
        CohortPicks want_picks;
        CohortResults want = genotype_cohort_sampled(other.unique_kmers, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, &want_picks);
        for (auto& sample : want)
            for (auto& kv : sample)
                for (GenotypingResult& r : kv.second) r.normalize();
        size_t compared = 0, no_call = 0, values = 0;
        for (const bool ignore_imputed : {false, true}) {
            CohortPicks got_picks;
            const CohortFields got = genotype_cohort_sampled_record_fields(m.unique_kmers, graphs, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false,
                                                                           0.00001L, 0, ignore_imputed, ignore_imputed ? nullptr : &got_picks);
            compare_lines(graphs, want, got, ignore_imputed, &compared, &no_call, &values);
            if (!ignore_imputed) CHECK(same_picks(got_picks, want_picks));
        }
        CHECK(serialize_unique_kmers_map(m) == serialize_unique_kmers_map(index));   // the objects are not touched
        CHECK(compared == 4 * records && records > 100 && values > 3 * compared);
        std::printf("  %zu records (%zu merged bubbles, %zu records with an undefined allele), %zu lines compared, %zu GL values, %zu lines without a call\n",
                    records, merged, with_undefined, compared, values, no_call);
    });

    run("Graph::genotypes_records(genotype_cohort_sampled_reads_record_fields) = Graph::genotypes_records(genotype_cohort_sampled_reads + normalize); batch 1 = batch 2", [&] {
        UniqueKmersMap m = fresh(), other = fresh();
        CohortPicks want_picks;
        CohortResults want = genotype_cohort_sampled_reads(other, prefix, reads, coverage, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, 2, &want_picks);
        for (auto& sample : want)
            for (auto& kv : sample)
                for (GenotypingResult& r : kv.second) r.normalize();
        size_t compared = 0, no_call = 0, values = 0;
        for (const bool ignore_imputed : {false, true}) {
            CohortPicks got_picks;
            const CohortFields got = genotype_cohort_sampled_reads_record_fields(m, graphs, prefix, reads, coverage, panel_size, true, 10, 25000.0L, &probs, 1.26, false,
                                                                                 0.00001L, 0, ignore_imputed ? 1 : 2, ignore_imputed, &got_picks);
            compare_lines(graphs, want, got, ignore_imputed, &compared, &no_call, &values);
            CHECK(same_picks(got_picks, want_picks));
        }
        CHECK(serialize_unique_kmers_map(m) == serialize_unique_kmers_map(index));
        CHECK(compared == 4 * records && values > 3 * compared);
        std::printf("  %zu lines compared, %zu GL values, %zu lines without a call\n", compared, values, no_call);
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
