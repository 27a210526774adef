// test_subsets_records.cpp — pangenie::genotype_subsets_record_fields (pangenie_amd/host/graph_io.hpp: the `-a` flow to VCF
// lines, the sample column per record formed on the device from the combined bins) against the route it spares: the lines of
// Graph::genotypes_records on genotype_subsets(..., normalize = true), text for text, with and without ignore_imputed, for two
// and for three subsets of the panel's paths.
//   test_subsets_records gpu <UniqueKmersMap archive with read counts> <Graph archive of its chromosome>
//                            (tests/golden/region_UniqueKmersList.cereal, tests/golden/index_chr1_Graph.cereal)
#include <algorithm>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../pangenie_amd/host/cereal_io.hpp"
#include "../../pangenie_amd/host/graph_io.hpp"

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
    if (argc < 4 || std::string(argv[1]) != "gpu") { std::printf("usage: test_subsets_records gpu <UniqueKmersMap archive with read counts> <Graph archive>\n"); return 2; }
    UniqueKmersMap m = load_unique_kmers_map(argv[2]);
    ProbabilityTable probs(1, 160, 80, 0.01L);
    unsigned short n_paths = 0;
    std::map<std::string, Graph> graphs;
    for (auto& kv : m.unique_kmers) {
        if (!kv.second.empty()) n_paths = kv.second[0]->get_nr_paths();
        graphs[kv.first] = Graph::load(argv[3]);
    }
    std::printf("  %zu chromosomes, %u paths\n", m.unique_kmers.size(), (unsigned)n_paths);
    // two subsets: the even paths and the odd ones; three: those and the first half once more
    std::vector<std::vector<unsigned short>> three(3);
    for (unsigned short p = 0; p < n_paths; ++p) three[p % 2].push_back(p);
    for (unsigned short p = 0; p < (n_paths + 1) / 2; ++p) three[2].push_back(p);
    std::vector<std::vector<unsigned short>> two(three.begin(), three.begin() + 2);

    for (const std::vector<std::vector<unsigned short>>* subsets : {&two, &three}) {
        const std::string name = std::string("the lines from the record fields = the lines from genotype_subsets + normalize, ") + (subsets == &two ? "two" : "three") + " subsets";
        run(name.c_str(), [&] {
            CHECK(n_paths >= 4);
            auto want = genotype_subsets(m.unique_kmers, *subsets, &probs, 1.26, false, 0.00001L, 0, true);
            size_t compared = 0, widest = 0, with_call = 0, values = 0, finite = 0;
            for (const bool ignore_imputed : {false, true}) {
                const auto got = genotype_subsets_record_fields(m.unique_kmers, graphs, *subsets, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
                CHECK(got.size() == want.size());
                for (auto& kv : want) {
                    const Graph& graph = graphs.at(kv.first);
                    const std::vector<std::string> lines = graph.genotypes_records(kv.second, ignore_imputed);
                    const auto found = got.find(kv.first);
                    CHECK(found != got.end());
                    if (found == got.end()) continue;
                    const SampledRecordFields& f = found->second;
                    CHECK(f.coverage.size() == kv.second.size() && f.unique_kmers.size() == kv.second.size());
                    for (size_t v = 0; v < kv.second.size() && v < f.coverage.size(); ++v)
                        CHECK(f.coverage[v] == kv.second[v].coverage() && f.unique_kmers[v] == kv.second[v].nr_unique_kmers());
                    const std::vector<std::string> ours = graph.genotypes_records(f.fields, f.coverage, f.unique_kmers, ignore_imputed);
                    CHECK(ours.size() == lines.size() && f.fields.calls.size() == lines.size() && f.fields.gl_off.size() == lines.size() + 1);
                    for (size_t r = 0; r < lines.size() && r < ours.size(); ++r) {
                        CHECK(ours[r] == lines[r]);
                        if (ours[r] != lines[r] && g_failed <= 20) std::printf("    record %zu:\n      %s\n      %s\n", r, ours[r].c_str(), lines[r].c_str());
                        compared += 1;
                        with_call += lines[r].find("\t.:.:") == std::string::npos;
                    }
                    for (const pg_gl& x : f.fields.gl) { values += 1; finite += x.mant != 0; CHECK(!(x.mant == 0 && x.exp10 == PG_GL_DEFERRED)); }
                    for (const GenotypeCall& c : f.fields.calls) CHECK(!c.deferred);   // (these likelihoods are nowhere near 2^-16300)
                    if (!ignore_imputed)
                        for (size_t v = 0; v < graph.size(); ++v) widest = std::max(widest, graph.get_variant(v).nr_of_alleles());
                }
            }
            CHECK(compared >= 4 && with_call >= 2 && values >= 3 * compared && finite > 0);
            CHECK(widest > 5);    // the fixture's bubbles hold tens of alleles: the wave-per-record kernels form these records
            std::printf("  %zu lines compared (%zu with a call), %zu GL values (%zu finite), widest bubble %zu alleles\n", compared, with_call, values, finite, widest);
        });
    }

    run("a missing graph, a graph of another size and no subsets are refused; no chromosomes are nothing to do", [&] {
        std::string what;
        std::map<std::string, Graph> none;
        try { genotype_subsets_record_fields(m.unique_kmers, none, two, &probs); } catch (const std::exception& e) { what = e.what(); }
        CHECK(what.find("genotype_subsets_record_fields: no graph of ") == 0);
        what.clear();
        std::map<std::string, Graph> empty_graphs;
        for (auto& kv : m.unique_kmers) empty_graphs[kv.first] = Graph();
        try { genotype_subsets_record_fields(m.unique_kmers, empty_graphs, two, &probs); } catch (const std::exception& e) { what = e.what(); }
        CHECK(what.find("genotype_subsets_record_fields: no graph of ") == 0);
        what.clear();
        try { genotype_subsets_record_fields(m.unique_kmers, graphs, {}, &probs); } catch (const std::exception& e) { what = e.what(); }
        CHECK(what == "genotype_subsets_record_fields: no subsets of paths");
        std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> no_chromosomes;
        CHECK(genotype_subsets_record_fields(no_chromosomes, graphs, two, &probs).empty());
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
