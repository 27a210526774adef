// test_panel_host.cpp — the sampled-panel VCF of a sampled cohort from the device (pangenie_amd/host/graph_io.hpp:
// sample_cohort_panel_text, sample_cohort_panel_lines, Graph::sampled_panel_records(RecordText),
// Graph::write_sampled_panel(RecordLines)) against the host's own route: genotype_cohort_sampled(..., &sampled),
// the picks applied to fresh UniqueKmers objects as the reference applies them (update_paths, then get_path_ids + size():
// src/commands.cpp:994-1005), SampledPanels, Graph::sampled_panel_records.  Line for line.
//   test_panel_host cpu
//       the drivers refuse a missing graph before any job and do nothing without samples; no device
//   test_panel_host counted <UniqueKmersMap archive with read counts> <Graph archive> <cov min> <cov max> <count max> <panel size>
//       the counts the archive holds as two samples; then the same with a graph whose first REF is of undefined sequence:
//       the host route inside the drivers
#include <cstdio>
#include <cstdlib>
#include <fstream>
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
static std::string file_bytes(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

// the graph of the fixture with the REF of its first record replaced by a sequence that holds an N
static Graph with_undefined_reference(const Graph& graph) {
    const RecordPlan plan = graph.record_plan();
    std::vector<Variant> variants;
    for (size_t i = 0; i < graph.size(); ++i) {
        const Variant& v = graph.get_variant(i);
        if (v.nr_of_records() != 1) throw std::runtime_error("with_undefined_reference: a bubble of one record each is expected");
        std::vector<std::string> alleles = v.records(nullptr).at(0).alleles;
        if (i == 0) alleles[0] = std::string(alleles[0].size(), 'N');
        std::vector<std::vector<unsigned short>> combinations;
        for (size_t a = 0; a < v.nr_of_alleles(); ++a) combinations.push_back({plan.map.at(plan.map_off.at(i) + a)});
        std::vector<unsigned short> paths;
        for (size_t p = 0; p < v.nr_of_paths(); ++p) paths.push_back(v.get_allele_on_path(p));
        variants.push_back(Variant::from_parts(v.get_chromosome(), v.get_start_position(), "", "", {alleles}, {}, combinations, paths, false));
    }
    return Graph::from_parts(graph.get_chromosome(), graph.get_kmer_size(), graph.reference_added(), variants, graph.variant_ids());
}

// what the host makes of a sample's picks on one chromosome: the reference's update_unique_kmers, then its SampledPanels
static std::vector<SampledPanel> panels_of(std::vector<std::shared_ptr<UniqueKmers>>& bubbles, const SampledPaths& picks) {
    std::vector<SampledPanel> panels(bubbles.size());
    for (size_t v = 0; v < bubbles.size(); ++v) {
        std::vector<unsigned short> ids;
        for (const std::vector<size_t>& path : picks.sampled_paths) ids.push_back((unsigned short)path.at(v));
        bubbles[v]->update_paths(ids);
        std::vector<unsigned short> paths;
        bubbles[v]->get_path_ids(paths, panels[v].path_to_allele);
        panels[v].unique_kmers = bubbles[v]->size();
    }
    return panels;
}

static void drivers_against_the_host(const std::function<UniqueKmersMap()>& fresh, const std::map<std::string, Graph>& graphs, const std::vector<SampleCounts>& counts,
                                     ProbabilityTable& probs, size_t panel_size, size_t records, const char* what, bool host_route) {
    run(what, [&] {
        UniqueKmersMap a = fresh(), b = fresh(), c = fresh();
        std::vector<std::map<std::string, SampledPaths>> picks;
        genotype_cohort_sampled(a.unique_kmers, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, &picks);
        const auto text = sample_cohort_panel_text(b.unique_kmers, graphs, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0);
        const auto lines = sample_cohort_panel_lines(c.unique_kmers, graphs, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0);
        CHECK(picks.size() == counts.size() && text.size() == counts.size() && lines.size() == counts.size());
        size_t compared = 0, dots = 0, bytes = 0;
        for (size_t s = 0; s < counts.size() && s < text.size() && s < lines.size() && s < picks.size(); ++s)
            for (const auto& kv : graphs) {
                const Graph& graph = kv.second;
                CHECK(graph.has_undefined_reference_allele() == host_route);
                UniqueKmersMap own = fresh();
                const std::vector<SampledPanel> panels = panels_of(own.unique_kmers.at(kv.first), picks[s].at(kv.first));
                const std::vector<std::string> want = graph.sampled_panel_records(panels);
                const RecordText& t = text[s].at(kv.first);
                const RecordLines& l = lines[s].at(kv.first);
                const std::vector<std::string> got = graph.sampled_panel_records(t);
                CHECK(got.size() == want.size() && want.size() == graph.record_plan().nr_of_records());
                CHECK(l.off.size() == want.size() + 1 && l.off[0] == 0 && l.off.back() == l.bytes.size());
                if (l.off.size() != want.size() + 1 || got.size() != want.size()) continue;
                size_t ok = 0;
                std::string joined;
                for (size_t r = 0; r < want.size(); ++r) {
                    const bool same = got[r] == want[r] && l.off[r] == joined.size() && l.bytes.compare(l.off[r], l.off[r + 1] - l.off[r], want[r] + '\n') == 0;
                    if (!same && g_failed <= 20) std::printf("    record %zu:\n      %s\n      %s\n", r, got[r].c_str(), want[r].c_str());
                    ok += same;
                    joined += want[r] + '\n';
                    dots += want[r].find("\t.") != std::string::npos;
                    CHECK(want[r].find("\tGT\t") != std::string::npos);
                }
                CHECK(ok == want.size() && l.bytes == joined);
                compared += want.size();
                bytes += l.bytes.size();
                for (size_t v = 0; v < panels.size(); ++v) CHECK(t.unique_kmers.at(v) == panels[v].unique_kmers);
                // the file: the header, then the body in one write; read back equal to the host's file
                const std::string path = "test_panel_host." + kv.first + ".tmp.vcf";
                graph.write_sampled_panel(path, panels, true);
                const std::string want_file = file_bytes(path);
                graph.write_sampled_panel(path, l, true, panel_size + 1);
                const std::string got_file = file_bytes(path);
                std::remove(path.c_str());
                CHECK(got_file == want_file && got_file.size() > l.bytes.size());
            }
        CHECK(compared == counts.size() * records && bytes > 20 * compared);
        std::printf("  %zu lines compared, %zu bytes, %zu lines with a `.` haplotype\n", compared, bytes, dots);
    });
}

int main(int argc, char** argv) {
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (mode == "cpu") {
        run("the drivers refuse a missing graph before any job, and do nothing without samples", [] {
            std::vector<unsigned short> alleles = {0, 1};
            std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> chromosomes;
            chromosomes["chr2"] = {std::make_shared<BiallelicUniqueKmers>(99, alleles)};
            std::map<std::string, Graph> none;
            std::vector<SampleCounts> samples(1);
            ProbabilityTable probs(1, 160, 80, 0.01L);
            CHECK(what_of([&] { sample_cohort_panel_text(chromosomes, none, samples, 7, true, 10, 25000.0L, &probs); }).find("no graph of chr2") != std::string::npos);
            CHECK(what_of([&] { sample_cohort_panel_lines(chromosomes, none, samples, 7, true, 10, 25000.0L, &probs); }).find("no graph of chr2") != std::string::npos);
            CHECK(sample_cohort_panel_text(chromosomes, none, {}, 7, true, 10, 25000.0L, &probs).empty());
            CHECK(sample_cohort_panel_lines(chromosomes, none, {}, 7, true, 10, 25000.0L, &probs).empty());
        });
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (mode != "counted" || argc < 8) {
        std::printf("usage: test_panel_host cpu | counted <archive> <graph> <cov min> <cov max> <count max> <panel size>\n");
        return 2;
    }
    const std::string archive = argv[2], graph_archive = argv[3];
    ProbabilityTable probs((unsigned)std::atoi(argv[4]), (unsigned)std::atoi(argv[5]), (unsigned)std::atoi(argv[6]), 0.01L);
    const size_t panel_size = (size_t)std::atoi(argv[7]);
    auto fresh = [&] { return load_unique_kmers_map(archive); };
    const UniqueKmersMap index = fresh();
    std::map<std::string, Graph> graphs, undefined_ref;
    size_t records = 0;
    for (const auto& kv : index.unique_kmers) {
        graphs[kv.first] = Graph::load(graph_archive);
        undefined_ref[kv.first] = with_undefined_reference(graphs[kv.first]);
        records += graphs[kv.first].record_plan().nr_of_records();
    }
    const SampleCounts one = SampleCounts::of(index.unique_kmers);
    drivers_against_the_host(fresh, graphs, {one, one}, probs, panel_size, records, "sample_cohort_panel_text / _lines = Graph::sampled_panel_records over the host's SampledPanels", false);
    drivers_against_the_host(fresh, undefined_ref, {one, one}, probs, panel_size, records, "a REF of undefined sequence (the host route)", true);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
