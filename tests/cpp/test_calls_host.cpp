// test_calls_host.cpp — pangenie::genotype_cohort_calls (pangenie_amd/host/pangenie_host.hpp) against the route it spares:
// genotype_cohort, then GenotypingResult::normalize / get_likeliest_genotype / get_genotype_quality per variant on the host.
// Every comparison is exact.
//   test_calls_host gpu <index prefix> <reads of sample 1> <reads of sample 2>
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
        if (!(cond)) { if (++g_failed <= 20) std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
static void run(const char* name, const std::function<void()>& f) {
    const int before = g_failed;
    try { f(); } catch (const std::exception& e) { ++g_failed; std::printf("  EXCEPTION in %s: %s\n", name, e.what()); }
    std::printf("%s %s\n", g_failed == before ? "ok  " : "FAIL", name);
}

int main(int argc, char** argv) {
    if (argc < 5 || std::string(argv[1]) != "gpu") { std::printf("usage: test_calls_host gpu <index prefix> <reads 1> <reads 2>\n"); return 2; }
    const std::string prefix = argv[2];
    const std::vector<std::string> both = {argv[3], argv[4]};
    const std::vector<size_t> coverage = {20, 17};

    run("genotype_cohort_calls = genotype_cohort + normalize / get_likeliest_genotype / get_genotype_quality, two samples", [&] {
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
        CHECK(!(counts[0].kmer_count == counts[1].kmer_count));
        ProbabilityTable probs(1, 160, 80, 0.01L);
        auto want = genotype_cohort(m.unique_kmers, counts, &probs, 1.26, false, 0.00001L, 0);
        const auto got = genotype_cohort_calls(m.unique_kmers, counts, &probs, 1.26, false, 0.00001L, 0);
        CHECK(got.size() == 2 && want.size() == 2);
        size_t variants = 0, called = 0, differ = 0, deferred = 0;
        for (size_t s = 0; s < want.size() && s < got.size(); ++s) {
            CHECK(got[s].size() == want[s].size());
            for (auto& kv : want[s]) {
                const auto found = got[s].find(kv.first);
                CHECK(found != got[s].end() && found->second.size() == kv.second.size());
                if (found == got[s].end() || found->second.size() != kv.second.size()) continue;
                for (size_t v = 0; v < kv.second.size(); ++v) {
                    GenotypingResult& r = kv.second[v];
                    r.normalize();
                    const std::pair<int, int> g = r.get_likeliest_genotype();
                    const GenotypeCall& c = found->second[v];
                    const bool has = g.first >= 0 && g.second >= 0;
                    CHECK(c.allele_1 == (has ? g.first : -1) && c.allele_2 == (has ? g.second : -1));
                    CHECK(c.quality == (has ? r.get_genotype_quality((unsigned short)g.first, (unsigned short)g.second) : (size_t)0));
                    variants += 1; called += has; deferred += c.deferred;
                    if (s == 1) { const GenotypeCall& o = got[0].at(kv.first)[v]; differ += o.allele_1 != c.allele_1 || o.allele_2 != c.allele_2 || o.quality != c.quality; }
                }
            }
        }
        CHECK(variants > 100 && called > variants / 2 && differ > 0);
        CHECK(deferred == 0);   // (these likelihoods are nowhere near 2^-16300)
        std::printf("  %zu variants compared, %zu with a call, %zu differ between the samples\n", variants, called, differ);
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
