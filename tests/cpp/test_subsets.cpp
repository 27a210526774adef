// test_subsets.cpp — pangenie::genotype_subsets and genotype_subsets_calls (pangenie_amd/host/pangenie_host.hpp: the
// reference's `-a` flow as one device job, the subsets combined on the device) against the route they spare: one
// HMM(..., only_paths, normalize = false) per subset, HMM::combine_likelihoods in the order of the subsets, normalize().
// Every long double is compared with ==, every key set is equal, unique_kmers and coverage are equal.
//   test_subsets gpu <UniqueKmersMap archive with read counts>      (tests/golden/region_UniqueKmersList.cereal)
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../pangenie_amd/host/cereal_io.hpp"

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

typedef std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> Chromosomes;
typedef std::map<std::string, std::vector<GenotypingResult>> SubsetResults;

// the reference's route: one HMM per subset, added up in the order of `subsets`
static SubsetResults host_route(Chromosomes& chromosomes, std::vector<std::vector<unsigned short>> subsets, ProbabilityTable* probs, bool normalize) {
    SubsetResults out;
    for (auto& kv : chromosomes) {
        HMM total;
        for (size_t s = 0; s < subsets.size(); ++s) {
            HMM one(&kv.second, probs, true, false, 1.26, false, 0.00001L, &subsets[s], false);
            if (s == 0) total = one;
            else total.combine_likelihoods(one);
        }
        if (normalize) total.normalize();
        out[kv.first] = total.get_genotyping_result();
    }
    return out;
}

struct Tally { size_t variants = 0, keys = 0, nonzero = 0; };

static void compare(const SubsetResults& got, const SubsetResults& want, Tally* t) {
    CHECK(got.size() == want.size());
    for (const auto& kv : want) {
        const auto found = got.find(kv.first);
        CHECK(found != got.end() && found->second.size() == kv.second.size());
        if (found == got.end() || found->second.size() != kv.second.size()) continue;
        for (size_t v = 0; v < kv.second.size(); ++v) {
            const GenotypingResult &w = kv.second[v], &g = found->second[v];
            const auto &wl = w.get_stored_likelihoods(), &gl = g.get_stored_likelihoods();
            CHECK(wl.size() == gl.size());
            auto a = wl.begin();
            auto b = gl.begin();
            for (; a != wl.end() && b != gl.end(); ++a, ++b) {
                CHECK(a->first == b->first);
                CHECK(a->second == b->second);
                t->keys += 1;
                t->nonzero += a->second > 0.0L;
            }
            CHECK(w.nr_unique_kmers() == g.nr_unique_kmers() && w.coverage() == g.coverage());
            t->variants += 1;
        }
    }
}

int main(int argc, char** argv) {
    if (argc < 3 || std::string(argv[1]) != "gpu") { std::printf("usage: test_subsets gpu <UniqueKmersMap archive with read counts>\n"); return 2; }
    UniqueKmersMap m = load_unique_kmers_map(argv[2]);
    ProbabilityTable probs(1, 160, 80, 0.01L);
    unsigned short n_paths = 0;
    for (auto& kv : m.unique_kmers)
        if (!kv.second.empty()) n_paths = kv.second[0]->get_nr_paths();
    std::printf("  %zu chromosomes, %u paths\n", m.unique_kmers.size(), (unsigned)n_paths);
    // subsets of the size the -a flow uses: four runs of 16 paths (the last one 15) out of a wide panel, as they come;
    // a narrow panel: the even paths, the odd ones, and the first half once more
    std::vector<std::vector<unsigned short>> subsets;
    if (n_paths >= 64) {
        for (const unsigned short first : {(unsigned short)0, (unsigned short)16, (unsigned short)(n_paths / 2), (unsigned short)(n_paths - 15)}) {
            subsets.emplace_back();
            for (unsigned short p = first; p < first + 16 && p < n_paths; ++p) subsets.back().push_back(p);
        }
    } else {
        subsets.resize(3);
        for (unsigned short p = 0; p < n_paths; ++p) subsets[p % 2].push_back(p);
        for (unsigned short p = 0; p < (n_paths + 1) / 2; ++p) subsets[2].push_back(p);
    }

    run("genotype_subsets = HMM per subset, combine_likelihoods in the order of the subsets, normalize", [&] {
        CHECK(n_paths >= 4);
        for (const bool normalize : {true, false}) {
            Tally t;
            compare(genotype_subsets(m.unique_kmers, subsets, &probs, 1.26, false, 0.00001L, 0, normalize), host_route(m.unique_kmers, subsets, &probs, normalize), &t);
            CHECK(t.variants > 0 && t.keys > t.variants && t.nonzero > t.variants / 2);
            std::printf("  normalize = %d: %zu variants, %zu keys (%zu nonzero) compared with ==\n", (int)normalize, t.variants, t.keys, t.nonzero);
        }
    });

    run("the order of the subsets is the order of the additions", [&] {
        std::vector<std::vector<unsigned short>> reversed(subsets.rbegin(), subsets.rend());
        Tally t;
        compare(genotype_subsets(m.unique_kmers, reversed, &probs, 1.26, false, 0.00001L, 0, false), host_route(m.unique_kmers, reversed, &probs, false), &t);
        CHECK(t.keys > 0);
        // one subset alone: the chain's own likelihoods
        std::vector<std::vector<unsigned short>> one(1, subsets[0]);
        Tally t1;
        compare(genotype_subsets(m.unique_kmers, one, &probs, 1.26, false, 0.00001L, 0, true), host_route(m.unique_kmers, one, &probs, true), &t1);
        CHECK(t1.keys > 0);
    });

    run("genotype_subsets_calls = normalize / get_likeliest_genotype / get_genotype_quality on genotype_subsets", [&] {
        SubsetResults want = genotype_subsets(m.unique_kmers, subsets, &probs, 1.26, false, 0.00001L, 0, false);
        const auto got = genotype_subsets_calls(m.unique_kmers, subsets, &probs, 1.26, false, 0.00001L, 0);
        CHECK(got.size() == want.size());
        size_t variants = 0, called = 0, deferred = 0;
        for (auto& kv : want) {
            const auto found = got.find(kv.first);
            CHECK(found != got.end() && found->second.size() == kv.second.size());
            if (found == got.end() || found->second.size() != kv.second.size()) continue;
            for (size_t v = 0; v < kv.second.size(); ++v) {
                GenotypingResult& r = kv.second[v];
                r.normalize();
                const std::pair<int, int> g = r.get_likeliest_genotype();
                const GenotypeCall& c = found->second[v];
                const bool has = g.first >= 0 && g.second >= 0;
                CHECK(c.allele_1 == (has ? g.first : -1) && c.allele_2 == (has ? g.second : -1));
                CHECK(c.quality == (has ? r.get_genotype_quality((unsigned short)g.first, (unsigned short)g.second) : (size_t)0));
                variants += 1; called += has; deferred += c.deferred;
            }
        }
        CHECK(variants > 0 && called > 0);
        CHECK(deferred == 0);   // (these likelihoods are nowhere near 2^-16300)
        std::printf("  %zu variants compared, %zu with a call\n", variants, called);
    });

    run("no subsets are refused, no chromosomes are nothing to do", [&] {
        std::string what;
        try { genotype_subsets(m.unique_kmers, {}, &probs); } catch (const std::exception& e) { what = e.what(); }
        CHECK(what == "genotype_subsets: no subsets of paths");
        Chromosomes none;
        CHECK(genotype_subsets(none, subsets, &probs).empty() && genotype_subsets_calls(none, subsets, &probs).empty());
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
