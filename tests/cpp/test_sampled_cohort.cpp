// test_sampled_cohort.cpp — pangenie::genotype_cohort_sampled (pangenie_amd/host/pangenie_host.hpp) on the GPU against the
// reference's per-sample sequence through the same host interface: for every sample, objects holding that sample's counts,
// HaplotypeSampler(&objects, size, ...) and HMM(&objects, ..., normalize = false) — results, bit for bit, and sampled paths.
//
//   test_sampled_cohort gpu
#include <cstdio>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../pangenie_amd/host/pangenie_host.hpp"

using namespace pangenie;
using Chromosomes = std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        ++g_checks;                                                  \
        if (!(cond)) {                                               \
            ++g_failed;                                              \
            std::printf("FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                \
            std::printf("\n");                                       \
        }                                                            \
    } while (0)

// one chromosome of a seeded panel: n_paths paths as a mosaic of 8 founders, 2..max_alleles alleles per object, a few
// undefined alleles, up to 12 k-mers per object (counts are set per sample afterwards)
static std::vector<std::shared_ptr<UniqueKmers>> make_chromosome(unsigned seed, size_t V, size_t P, unsigned max_alleles) {
    std::mt19937 rng(seed);
    auto uni = [&](unsigned lo, unsigned hi) { return lo + (unsigned)(rng() % (hi - lo + 1)); };
    std::vector<std::shared_ptr<UniqueKmers>> out;
    std::vector<unsigned> mosaic(P);
    for (auto& m : mosaic) m = uni(0, 7);
    size_t pos = 1000;
    for (size_t v = 0; v < V; ++v) {
        pos += uni(1, 3000);
        const unsigned A = uni(2, max_alleles);
        if (uni(0, 9) < 3)
            for (size_t k = 0; k < P / 16 + 1; ++k) mosaic[uni(0, (unsigned)P - 1)] = uni(0, 7);
        unsigned founders[8];
        for (auto& f : founders) f = uni(0, A - 1);
        std::vector<unsigned short> alleles(P);
        for (size_t p = 0; p < P; ++p) alleles[p] = (unsigned short)(uni(0, 19) == 0 ? uni(0, A - 1) : founders[mosaic[p]]);
        std::shared_ptr<UniqueKmers> uk;
        if (A > 2) uk = std::make_shared<MultiallelicUniqueKmers>(pos, alleles);
        else uk = std::make_shared<BiallelicUniqueKmers>(pos, alleles);
        std::vector<unsigned short> ids;
        uk->get_allele_ids(ids);
        for (unsigned short a : ids)
            if (uni(0, 49) == 0) uk->set_undefined_allele(a);
        for (unsigned short a : ids)
            for (unsigned k = uni(0, 3); k > 0 && uk->size() < 12; --k) {
                std::vector<unsigned short> on{a};
                uk->insert_kmer(0, on);
            }
        uk->set_coverage(20);
        out.push_back(uk);
    }
    return out;
}

static Chromosomes make_index() {
    Chromosomes c;
    c["chr1"] = make_chromosome(11, 90, 120, 4);
    c["chr2"] = make_chromosome(12, 60, 40, 7);
    return c;
}

int main(int argc, char** argv) {
    if (argc < 2 || std::string(argv[1]) != "gpu") { std::printf("usage: test_sampled_cohort gpu\n"); return 2; }
    std::mt19937 rng(5);
    const unsigned short count_values[] = {0, 1, 2, 3, 5, 9};
    const size_t n_samples = 3, size = 15;
    Chromosomes index = make_index();
    std::vector<SampleCounts> samples(n_samples);
    for (size_t s = 0; s < n_samples; ++s)
        for (auto& kv : index) {
            for (auto& u : kv.second) {
                for (size_t k = 0; k < u->size(); ++k) samples[s].kmer_count[kv.first].push_back(count_values[(rng() + s) % 6]);
                samples[s].coverage[kv.first].push_back((uint16_t)(5 + rng() % 35));
            }
        }
    ProbabilityTable probs(1, 160, 80, 0.01L);
    for (int add_reference = 0; add_reference < 2; ++add_reference) {
        std::vector<std::map<std::string, SampledPaths>> sampled;
        auto got = genotype_cohort_sampled(index, samples, size, add_reference != 0, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, &sampled);
        CHECK(got.size() == n_samples && sampled.size() == n_samples, "sizes");
        std::vector<std::string> first_paths;
        for (size_t s = 0; s < n_samples; ++s) {
            Chromosomes own = make_index();   // the same index, holding this sample's numbers (fill_read_kmercounts)
            for (auto& kv : own) {
                size_t i = 0, v = 0;
                for (auto& u : kv.second) {
                    for (size_t k = 0; k < u->size(); ++k) u->update_readcount(k, samples[s].kmer_count[kv.first][i++]);
                    u->set_coverage(samples[s].coverage[kv.first][v++]);
                }
                HaplotypeSampler hs(&kv.second, size, 1.26, 25000.0L, nullptr, add_reference != 0, "", "None", 10);
                HMM hmm(&kv.second, &probs, true, false, 1.26, false, 0.00001L, nullptr, false);
                const std::vector<GenotypingResult> want = hmm.get_genotyping_result();
                const std::vector<GenotypingResult>& res = got[s][kv.first];
                CHECK(res.size() == want.size(), "s%zu %s: %zu results, want %zu", s, kv.first.c_str(), res.size(), want.size());
                for (size_t x = 0; x < res.size() && x < want.size(); ++x) {
                    CHECK(res[x].get_stored_likelihoods() == want[x].get_stored_likelihoods(), "s%zu %s variant %zu likelihoods", s, kv.first.c_str(), x);
                    CHECK(res[x].nr_unique_kmers() == want[x].nr_unique_kmers() && res[x].coverage() == want[x].coverage(),
                          "s%zu %s variant %zu k-mers / coverage", s, kv.first.c_str(), x);
                }
                const SampledPaths sp = hs.get_sampled_paths();
                CHECK(sampled[s][kv.first].sampled_paths == sp.sampled_paths, "s%zu %s sampled paths", s, kv.first.c_str());
                CHECK(sp.sampled_paths.size() == size + (size_t)add_reference, "s%zu %s number of paths", s, kv.first.c_str());
                if (kv.first == "chr1") {
                    std::string key;
                    for (auto& p : sp.sampled_paths) for (size_t id : p) key += std::to_string(id) + ",";
                    first_paths.push_back(key);
                }
            }
        }
        CHECK(first_paths.size() == n_samples && (first_paths[0] != first_paths[1] || first_paths[1] != first_paths[2]),
              "the samples picked the same paths: the test does not tell them apart");
    }
    // a sample that does not fit the index
    std::vector<SampleCounts> bad = {samples[0]};
    bad[0].kmer_count["chr2"].pop_back();
    bool threw = false;
    try { genotype_cohort_sampled(index, bad, size, true, 10, 25000.0L, &probs); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw, "a sample with too few counts must be refused");
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
