// test_count_plan.cpp — pangenie::DeviceCountPlan and genotype_cohort_reads (pangenie_amd/host/kmer_counts.hpp) against the host
// route they replace: fill_read_kmercounts[_all] over a TargetedKmerCounter, SampleCounts::of, genotype_cohort.  Every
// comparison is exact.
//   test_count_plan gpu <golden dir> [<index prefix> <reads of sample 1> <reads of sample 2>]
// <index prefix>: what `test_host index` wrote for a pangenome of tools/simulate_pangenome.py.
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../pangenie_amd/host/cereal_io.hpp"
#include "../../pangenie_amd/host/kmer_counts.hpp"

using namespace pangenie;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        ++g_checks;                                                                       \
        if (!(cond)) { ++g_failed; std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
static void run(const char* name, const std::function<void()>& f) {
    const int before = g_failed;
    try { f(); } catch (const std::exception& e) { ++g_failed; std::printf("  EXCEPTION in %s: %s\n", name, e.what()); }
    std::printf("%s %s\n", g_failed == before ? "ok  " : "FAIL", name);
}
static std::vector<unsigned char> read_file(const std::string& path) {
    std::vector<unsigned char> bytes;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return bytes;
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    return bytes;
}
static std::string thrown_by(const std::function<void()>& f) {
    try { f(); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}
static bool same_results(const std::vector<std::map<std::string, std::vector<GenotypingResult>>>& got,
                         const std::vector<std::map<std::string, std::vector<GenotypingResult>>>& want, size_t* variants) {
    if (got.size() != want.size()) return false;
    for (size_t s = 0; s < got.size(); ++s) {
        if (got[s].size() != want[s].size()) return false;
        for (const auto& kv : want[s]) {
            const auto found = got[s].find(kv.first);
            if (found == got[s].end() || found->second.size() != kv.second.size()) return false;
            for (size_t v = 0; v < kv.second.size(); ++v) {
                const GenotypingResult &g = found->second[v], &w = kv.second[v];
                if (!(g.get_stored_likelihoods() == w.get_stored_likelihoods()) || g.nr_unique_kmers() != w.nr_unique_kmers() || g.coverage() != w.coverage()) return false;
                *variants += 1;
            }
        }
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3 || std::string(argv[1]) != "gpu") { std::printf("usage: test_count_plan gpu <golden dir> [<index prefix> <reads 1> <reads 2>]\n"); return 2; }
    const std::string golden = argv[2];

    run("the golden index: DeviceCountPlan::fill_into = the reference's counted archive byte for byte", [&] {
        const std::string reads = golden + "/region-reads.fa";
        const UniqueKmersMap want = load_unique_kmers_map(golden + "/region_UniqueKmersList.cereal");
        const std::vector<unsigned char> want_bytes = read_file(golden + "/region_UniqueKmersList.cereal");
        CHECK(!want_bytes.empty());
        UniqueKmersMap m = load_unique_kmers_map(golden + "/index_UniqueKmersMap.cereal");
        DeviceKmerCounter counter(m.kmersize);
        DeviceCountPlan plan(counter, m, golden + "/index", true);
        CHECK(plan.chromosomes() == std::vector<std::string>{"chr1"} && plan.unique_kmers() > 0 && plan.flanking_kmers() > 0);
        counter.count(reads);
        plan.fill_into(&m, 18);
        CHECK(plan.last_fill_ms() > 0.0);
        m.runtimes = want.runtimes;
        m.sampling_runtimes = want.sampling_runtimes;
        CHECK(serialize_unique_kmers_map(m) == want_bytes);
        // the same numbers as arrays, and as what the host route leaves in the objects
        const SampleCounts got = plan.fill(18);
        const SampleCounts of = SampleCounts::of(want.unique_kmers);
        CHECK(got.kmer_count == of.kmer_count && got.coverage == of.coverage);
        // the next sample: no reads at all -> counts 0, coverage = the given one
        counter.reset_counts();
        const SampleCounts none = plan.fill(7);
        for (uint16_t c : none.kmer_count.at("chr1")) CHECK(c == 0);
        for (uint16_t c : none.coverage.at("chr1")) CHECK(c == 7);
        // targets after the plan froze the table are refused as after a count
        CHECK(thrown_by([&] { counter.add_target(std::string(31, 'A')); }) == "DeviceKmerCounter: targets must be registered before the reads are counted");
    });

    run("the constructor's checks: lines against variants, positions, missing table, unregistered k-mers", [&] {
        const UniqueKmersMap m = load_unique_kmers_map(golden + "/index_UniqueKmersMap.cereal");
        {
            UniqueKmersMap fewer = m;
            fewer.unique_kmers["chr1"].pop_back();
            DeviceKmerCounter c(m.kmersize);
            CHECK(thrown_by([&] { DeviceCountPlan p(c, fewer, golden + "/index", true); }) == "DeviceCountPlan: more lines than variants");
        }
        {
            UniqueKmersMap more = m;
            more.unique_kmers["chr1"].push_back(more.unique_kmers["chr1"].back());
            DeviceKmerCounter c(m.kmersize);
            CHECK(thrown_by([&] { DeviceCountPlan p(c, more, golden + "/index", true); }).rfind("DeviceCountPlan: fewer lines than variants", 0) == 0);
        }
        {
            UniqueKmersMap swapped = m;
            std::swap(swapped.unique_kmers["chr1"][0], swapped.unique_kmers["chr1"][1]);
            DeviceKmerCounter c(m.kmersize);
            CHECK(thrown_by([&] { DeviceCountPlan p(c, swapped, golden + "/index", true); }).find("does not match the index") != std::string::npos);
        }
        {
            UniqueKmersMap other = m;
            other.unique_kmers["chrNone"] = other.unique_kmers["chr1"];
            DeviceKmerCounter c(m.kmersize);
            CHECK(thrown_by([&] { DeviceCountPlan p(c, other, golden + "/index", true); }) == "DeviceCountPlan: kmer file cannot be opened.");
        }
        {
            UniqueKmersMap own = m;
            DeviceKmerCounter strict(m.kmersize), lenient(m.kmersize, true);
            strict.add_target(std::string(31, 'A'));
            lenient.add_target(std::string(31, 'A'));
            const std::string said = thrown_by([&] { DeviceCountPlan p(strict, own, golden + "/index", false); });
            CHECK(said.find("contig 0, variant 0, unique k-mer 0") != std::string::npos && said.find("was not registered") != std::string::npos);
            DeviceCountPlan p(lenient, own, golden + "/index", false);
            const SampleCounts zero = p.fill(18);
            for (uint16_t c : zero.kmer_count.at("chr1")) CHECK(c == 0);
        }
    });

    if (argc >= 6) {
        const std::string prefix = argv[3];
        const std::vector<std::string> reads = {argv[4], argv[5]};
        const std::vector<size_t> coverage = {20, 17};
        // (a UniqueKmersMap copies its objects by pointer: every route loads its own)
        auto fresh = [&] { return load_unique_kmers_map(prefix + "_UniqueKmersMap.cereal"); };
        const UniqueKmersMap index = fresh();
        std::vector<SampleCounts> host_counts;

        run("a simulated pangenome, table k-mers registered (strict): fill() = fill_read_kmercounts_all + SampleCounts::of", [&] {
            for (size_t s = 0; s < 2; ++s) {
                UniqueKmersMap m = fresh();
                TargetedKmerCounter host(index.kmersize);
                for (const auto& kv : index.unique_kmers) host.add_targets_from_table(prefix + "_" + kv.first + "_kmers.tsv.gz");
                host.count(reads[s], 8);
                fill_read_kmercounts_all(&m, host, prefix, coverage[s], 8);
                host_counts.push_back(SampleCounts::of(m.unique_kmers));
            }
            UniqueKmersMap m = fresh();
            DeviceKmerCounter dev(index.kmersize);
            DeviceCountPlan plan(dev, m, prefix, true);
            size_t entries = 0, nonzero = 0;
            for (size_t s = 0; s < 2; ++s) {
                dev.reset_counts();
                dev.count(reads[s]);
                const SampleCounts got = plan.fill(coverage[s]);
                CHECK(got.kmer_count == host_counts[s].kmer_count);
                CHECK(got.coverage == host_counts[s].coverage);
                for (const auto& kv : got.kmer_count) for (uint16_t c : kv.second) { entries += 1; nonzero += c != 0; }
            }
            CHECK(entries > 1000 && nonzero > entries / 4);
            CHECK(!(host_counts[0].kmer_count == host_counts[1].kmer_count));
            std::printf("  %zu entries compared, %zu of them not 0\n", entries, nonzero);
        });

        run("the same, graph segments registered (lenient): fill() and fill_into()", [&] {
            UniqueKmersMap want = fresh(), m = fresh();
            TargetedKmerCounter host(index.kmersize, true);
            DeviceKmerCounter dev(index.kmersize, true);
            CHECK(host.add_targets_from_sequences(prefix + "_path_segments.fasta") == dev.add_targets_from_sequences(prefix + "_path_segments.fasta"));
            host.count(reads[0], 8);
            dev.count(reads[0]);
            fill_read_kmercounts_all(&want, host, prefix, coverage[0], 8);
            DeviceCountPlan plan(dev, m, prefix, false);
            const SampleCounts got = plan.fill(coverage[0]), of = SampleCounts::of(want.unique_kmers);
            CHECK(got.kmer_count == of.kmer_count && got.coverage == of.coverage);
            plan.fill_into(&m, coverage[0]);
            CHECK(serialize_unique_kmers_map(m) == serialize_unique_kmers_map(want));
        });

        run("genotype_cohort_reads = genotype_cohort on the host-filled SampleCounts, two samples, one batch and two", [&] {
            CHECK(host_counts.size() == 2);
            UniqueKmersMap m = fresh();
            ProbabilityTable probs(1, 160, 80, 0.01L);
            const auto want = genotype_cohort(m.unique_kmers, host_counts, &probs, 1.26, false, 0.00001L, 0);
            for (size_t batch : {2u, 1u}) {
                size_t variants = 0;
                const auto got = genotype_cohort_reads(m, prefix, reads, coverage, &probs, 1.26, false, 0.00001L, 0, batch);
                CHECK(same_results(got, want, &variants));
                CHECK(variants > 100);
            }
            CHECK(serialize_unique_kmers_map(m) == serialize_unique_kmers_map(index));   // the objects are not touched
        });
    }

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
