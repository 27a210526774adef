// test_record_calls_host.cpp — pangenie::genotype_cohort_record_calls (pangenie_amd/host/graph_io.hpp) against the route it
// spares: genotype_cohort, GenotypingResult::normalize, then Graph::genotypes_records — the VCF text.  For every VCF record
// the GT and GQ of the sample column equal the record's call, with and without ignore_imputed.  Every comparison is exact.
//   test_record_calls_host gpu <index prefix> <reads of sample 1> <reads of sample 2>
// <index prefix>: what `test_host index` wrote for a pangenome of tools/simulate_pangenome.py in which some records miss a
// panel haplotype, which becomes an allele of undefined sequence (tests/test_record_calls_host_gpu.py).
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

// GT and GQ of a record line's sample column `GT:GQ:GL:KC`: "0/1:37:..." or ".:.:..."
static GenotypeCall call_of_line(const std::string& line) {
    const std::string field = line.substr(line.rfind('\t') + 1);
    const size_t c1 = field.find(':'), c2 = field.find(':', c1 + 1);
    if (c1 == std::string::npos || c2 == std::string::npos) throw std::runtime_error("no GT:GQ in " + field);
    const std::string gt = field.substr(0, c1), gq = field.substr(c1 + 1, c2 - c1 - 1);
    GenotypeCall c;
    if (gt == ".") { if (gq != ".") throw std::runtime_error("GQ without GT in " + field); return c; }
    const size_t slash = gt.find('/');
    if (slash == std::string::npos) throw std::runtime_error("GT without / in " + field);
    c.allele_1 = std::atoi(gt.substr(0, slash).c_str());
    c.allele_2 = std::atoi(gt.substr(slash + 1).c_str());
    c.quality = (size_t)std::strtoull(gq.c_str(), nullptr, 10);
    return c;
}

int main(int argc, char** argv) {
    if (argc < 5 || std::string(argv[1]) != "gpu") { std::printf("usage: test_record_calls_host gpu <index prefix> <reads 1> <reads 2>\n"); return 2; }
    const std::string prefix = argv[2];
    const std::vector<std::string> both = {argv[3], argv[4]};
    const std::vector<size_t> coverage = {20, 17};

    run("genotype_cohort_record_calls = GT:GQ of genotype_cohort + normalize + Graph::genotypes_records, two samples", [&] {
        UniqueKmersMap m = load_unique_kmers_map(prefix + "_UniqueKmersMap.cereal");
        std::vector<SampleCounts> counts;
        {
            DeviceKmerCounter dev(m.kmersize);
            DeviceCountPlan plan(dev, m, prefix, true);
            for (size_t s = 0; s < 2; ++s) {
                dev.reset_counts();
                dev.count(both[s]);
                counts.push_back(plan.fill(coverage[s]));
            }
        }
        std::map<std::string, Graph> graphs;
        size_t merged = 0, with_undefined = 0, records = 0;
        for (const auto& kv : m.unique_kmers) {
            graphs[kv.first] = Graph::load(prefix + "_" + kv.first + "_Graph.cereal");
            const Graph& g = graphs[kv.first];
            const RecordPlan plan = g.record_plan();
            CHECK(plan.rec_off.size() == g.size() + 1 && plan.nr_of_records() == g.variant_ids().size());
            for (size_t v = 0; v < g.size(); ++v) {
                CHECK(plan.rec_off[v + 1] - plan.rec_off[v] == g.get_variant(v).nr_of_records());
                merged += g.get_variant(v).nr_of_records() >= 2;
            }
            for (size_t r = 0; r < plan.nr_of_records(); ++r) {
                bool undefined = false;
                for (uint32_t i = plan.vcf_off[r]; i < plan.vcf_off[r + 1]; ++i) undefined = undefined || plan.vcf_index[i] == 0xFFFF;
                with_undefined += undefined;
            }
            records += plan.nr_of_records();
        }
        // the input holds what this test is about
        CHECK(merged >= 1);
        CHECK(with_undefined >= 1);
        ProbabilityTable probs(1, 160, 80, 0.01L);
        auto want = genotype_cohort(m.unique_kmers, counts, &probs, 1.26, false, 0.00001L, 0);
        for (auto& sample : want)
            for (auto& kv : sample)
                for (GenotypingResult& r : kv.second) r.normalize();
        size_t compared = 0, called = 0, differ = 0, deferred = 0, dropped = 0;
        for (const bool ignore_imputed : {false, true}) {
            const auto got = genotype_cohort_record_calls(m.unique_kmers, graphs, counts, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
            CHECK(got.size() == 2 && want.size() == 2);
            for (size_t s = 0; s < want.size() && s < got.size(); ++s) {
                CHECK(got[s].size() == want[s].size());
                for (auto& kv : want[s]) {
                    const std::vector<std::string> lines = graphs.at(kv.first).genotypes_records(kv.second, ignore_imputed);
                    const auto found = got[s].find(kv.first);
                    CHECK(found != got[s].end() && found->second.size() == lines.size());
                    if (found == got[s].end() || found->second.size() != lines.size()) continue;
                    for (size_t r = 0; r < lines.size(); ++r) {
                        const GenotypeCall text = call_of_line(lines[r]), &c = found->second[r];
                        CHECK(c.allele_1 == text.allele_1 && c.allele_2 == text.allele_2 && c.quality == text.quality);
                        if (!(c.allele_1 == text.allele_1 && c.allele_2 == text.allele_2 && c.quality == text.quality) && g_failed <= 20)
                            std::printf("    sample %zu record %zu: %d/%d:%zu, the VCF says %s\n", s, r, c.allele_1, c.allele_2, c.quality,
                                        lines[r].substr(lines[r].rfind('\t') + 1).c_str());
                        compared += 1; called += text.allele_1 >= 0; deferred += c.deferred;
                        if (ignore_imputed) dropped += text.allele_1 < 0;
                        if (s == 1 && !ignore_imputed) { const GenotypeCall& o = got[0].at(kv.first)[r]; differ += o.allele_1 != c.allele_1 || o.allele_2 != c.allele_2 || o.quality != c.quality; }
                    }
                }
            }
        }
        CHECK(compared == 4 * records && records > 100 && called > compared / 2 && differ > 0);
        CHECK(deferred == 0);   // (these likelihoods are nowhere near 2^-16300)
        std::printf("  %zu records (%zu merged bubbles, %zu records with an undefined allele), %zu comparisons, %zu with a call, %zu differ between the samples, "
                    "%zu without a call under ignore_imputed\n", records, merged, with_undefined, compared, called, differ, dropped);
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
