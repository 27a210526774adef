// test_sampled_reads.cpp — pangenie::genotype_cohort_sampled_reads and DeviceCountPlan::fill_device
// (pangenie_amd/host/kmer_counts.hpp) against the route they replace: DeviceCountPlan::fill to the host, SampleCounts,
// genotype_cohort_sampled.  Every comparison is exact.
//   test_sampled_reads gpu <index prefix> <reads of sample 1> <reads of sample 2>
// <index prefix>: what `test_host index` wrote for a pangenome of tools/simulate_pangenome.py.
#include <dlfcn.h>

#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pangenie_sampler.h"
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
static std::string thrown_by(const std::function<void()>& f) {
    try { f(); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}
// n uint16 entries of device memory on the host: hipMemcpy of the runtime the product library brought into the process (this
// test is compiled by g++, without the HIP headers)
static std::vector<uint16_t> from_device(const uint16_t* d, size_t n) {
    using copy_fn = int (*)(void*, const void*, size_t, int);
    static const copy_fn copy = (copy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    if (!copy) throw std::runtime_error("hipMemcpy is not in the process");
    std::vector<uint16_t> out(n);
    if (n && copy(out.data(), d, 2 * n, 2 /* hipMemcpyDeviceToHost */) != 0) throw std::runtime_error("hipMemcpy failed");
    return out;
}
using CohortResults = std::vector<std::map<std::string, std::vector<GenotypingResult>>>;
using CohortPicks = std::vector<std::map<std::string, SampledPaths>>;
static bool same_results(const CohortResults& got, const CohortResults& want, size_t* variants, size_t* with_likelihoods) {
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
                *with_likelihoods += w.get_stored_likelihoods().empty() ? 0 : 1;
            }
        }
    }
    return true;
}
static bool same_picks(const CohortPicks& got, const CohortPicks& want) {
    if (got.size() != want.size()) return false;
    for (size_t s = 0; s < got.size(); ++s) {
        if (got[s].size() != want[s].size()) return false;
        for (const auto& kv : want[s]) {
            const auto found = got[s].find(kv.first);
            if (found == got[s].end() || found->second.sampled_paths != kv.second.sampled_paths) return false;
        }
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 5 || std::string(argv[1]) != "gpu") { std::printf("usage: test_sampled_reads gpu <index prefix> <reads 1> <reads 2>\n"); return 2; }
    const std::string prefix = argv[2];
    const std::vector<std::string> reads = {argv[3], argv[4]};
    const std::vector<size_t> coverage = {20, 17};
    const size_t panel_size = 7;
    // (a UniqueKmersMap copies its objects by pointer: every route loads its own)
    auto fresh = [&] { return load_unique_kmers_map(prefix + "_UniqueKmersMap.cereal"); };
    const UniqueKmersMap index = fresh();
    std::vector<SampleCounts> host_counts;

    run("DeviceCountPlan::fill_device into a pg_sampler_counts, read back = fill()", [&] {
        UniqueKmersMap m = fresh();
        DeviceKmerCounter dev(index.kmersize);
        DeviceCountPlan plan(dev, m, prefix, true);
        const std::vector<std::string>& names = plan.chromosomes();
        const size_t C = names.size();
        std::vector<uint64_t> n_kmers(C);
        std::vector<uint32_t> n_variants(C);
        size_t c = 0;
        for (const auto& kv : m.unique_kmers) {   // (map order: the plan's)
            for (const auto& u : kv.second) n_kmers[c] += u->size();
            n_variants[c] = (uint32_t)kv.second.size();
            c += 1;
        }
        char err[512] = {0};
        pg_sampler_counts* counts = nullptr;
        CHECK(pg_sampler_counts_new(0, (uint32_t)C, n_kmers.data(), n_variants.data(), 2, &counts, err, sizeof err) == PG_OK);
        if (!counts) throw std::runtime_error(err);
        std::vector<uint16_t* const*> d_k(2, nullptr), d_c(2, nullptr);
        for (size_t s = 0; s < 2; ++s) {
            dev.reset_counts();
            dev.count(reads[s]);
            host_counts.push_back(plan.fill(coverage[s]));
            CHECK(pg_sampler_counts_rows(counts, (uint32_t)s, &d_k[s], &d_c[s], err, sizeof err) == PG_OK);
            plan.fill_device(coverage[s], d_k[s], d_c[s]);
        }
        CHECK(pg_sampler_counts_rows(counts, 2, nullptr, nullptr, err, sizeof err) == PG_ERR_INVALID);
        // both samples' rows are read only now: the second fill left the first sample's arrays alone
        size_t entries = 0, nonzero = 0;
        for (size_t s = 0; s < 2; ++s)
            for (c = 0; c < C; ++c) {
                const std::vector<uint16_t>&want_k = host_counts[s].kmer_count.at(names[c]), &want_c = host_counts[s].coverage.at(names[c]);
                CHECK(want_k.size() == n_kmers[c] && want_c.size() == n_variants[c]);
                CHECK(d_k[s][c] != nullptr && d_c[s][c] != nullptr);
                CHECK(from_device(d_k[s][c], want_k.size()) == want_k);
                CHECK(from_device(d_c[s][c], want_c.size()) == want_c);
                for (uint16_t x : want_k) { entries += 1; nonzero += x != 0; }
            }
        CHECK(pg_sampler_counts_destroy(counts) == PG_OK);
        CHECK(entries > 1000 && nonzero > entries / 4);
        CHECK(!(host_counts[0].kmer_count == host_counts[1].kmer_count));
        std::printf("  %zu entries compared, %zu of them not 0\n", entries, nonzero);
    });

    run("genotype_cohort_sampled_reads = genotype_cohort_sampled on the plan's host-filled SampleCounts; batch 1 = batch 2", [&] {
        CHECK(host_counts.size() == 2);
        UniqueKmersMap m = fresh(), other = fresh();
        ProbabilityTable probs(1, 160, 80, 0.01L);
        CohortPicks want_picks;
        const CohortResults want = genotype_cohort_sampled(other.unique_kmers, host_counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, &want_picks);
        CHECK(want_picks.size() == 2 && !same_picks({want_picks[0]}, {want_picks[1]}));   // the samples are told apart
        for (size_t batch : {2u, 1u}) {
            size_t variants = 0, with_likelihoods = 0;
            CohortPicks got_picks;
            const CohortResults got = genotype_cohort_sampled_reads(m, prefix, reads, coverage, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, batch, &got_picks);
            CHECK(same_results(got, want, &variants, &with_likelihoods));
            CHECK(variants > 100 && with_likelihoods > 100);
            CHECK(same_picks(got_picks, want_picks));
            for (const auto& kv : got_picks[0]) CHECK(kv.second.sampled_paths.size() == panel_size + 1);
        }
        // without the picks asked for: the same results
        size_t variants = 0, with_likelihoods = 0;
        CHECK(same_results(genotype_cohort_sampled_reads(m, prefix, reads, coverage, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, 2), want, &variants, &with_likelihoods));
        CHECK(serialize_unique_kmers_map(m) == serialize_unique_kmers_map(index));   // the objects are not touched
        CHECK(thrown_by([&] { genotype_cohort_sampled_reads(m, prefix, reads, {20}, panel_size, true, 10, 25000.0L, &probs); }) == "genotype_cohort_sampled_reads: one k-mer coverage per read file");
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
