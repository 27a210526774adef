// test_sampled_record_lines_host.cpp — the VCF lines of SAMPLED cohorts joined on the device over one slotted prefix per
// chromosome (pangenie_amd/host/graph_io.hpp: Graph::genotypes_fixed_columns_slotted, genotype_cohort_sampled_record_lines;
// kmer_counts.hpp: genotype_cohort_sampled_reads_record_lines) against the single-sample lines of
// Graph::genotypes_records(genotype_cohort_sampled_record_text).  Byte for byte.
//   test_sampled_record_lines_host cpu <Graph archive>
//       the slotted columns with the digits of uk put in at the slot are genotypes_fixed_columns(uk); no device
//   test_sampled_record_lines_host counted <UniqueKmersMap archive with read counts> <Graph archive> <cov min> <cov max> <count max> <panel size>
//       the counts the archive holds as two samples
//   test_sampled_record_lines_host gpu <index prefix> <reads of sample 1> <reads of sample 2>
//       two samples on the simulated pangenome of the other host tests, from counts and from reads
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

static void cpu_tests(const std::string& graph_archive) {
    const Graph graph = Graph::load(graph_archive);
    run("Graph::genotypes_fixed_columns_slotted: the digits of uk at the slot give genotypes_fixed_columns(uk)", [&] {
        std::vector<uint32_t> slot;
        const std::vector<std::string> slotted = graph.genotypes_fixed_columns_slotted(&slot);
        const size_t R = graph.record_plan().nr_of_records();
        CHECK(R >= 2 && slotted.size() == R && slot.size() == R);
        std::vector<size_t> bubble;   // of every record
        for (size_t v = 0; v < graph.size(); ++v) bubble.insert(bubble.end(), graph.get_variant(v).nr_of_records(), v);
        CHECK(bubble.size() == R);
        std::vector<std::vector<unsigned short>> uks(3, std::vector<unsigned short>(graph.size(), 0));   // all zero, random, 65535
        uint32_t x = 12345;
        for (size_t v = 0; v < graph.size(); ++v) {
            x = x * 1664525u + 1013904223u;
            uks[1][v] = (unsigned short)(x >> 16);
            uks[2][v] = 65535;
        }
        for (const std::vector<unsigned short>& uk : uks) {
            const std::vector<std::string> want = graph.genotypes_fixed_columns(uk);
            CHECK(want.size() == R);
            size_t ok = 0;
            for (size_t r = 0; r < R && r < want.size() && r < slotted.size() && r < bubble.size(); ++r) {
                CHECK(slot[r] <= slotted[r].size() && slot[r] >= 4 && slotted[r].compare(slot[r] - 4, 4, ";UK=") == 0);
                if (slot[r] > slotted[r].size()) continue;
                ok += slotted[r].substr(0, slot[r]) + std::to_string(uk[bubble[r]]) + slotted[r].substr(slot[r]) == want[r];
            }
            CHECK(ok == R);
        }
        CHECK(!what_of([&] { graph.genotypes_fixed_columns_slotted(nullptr); }).empty());
    });
    run("genotype_cohort_sampled_record_lines refuses a missing graph before any job, and does nothing without samples", [] {
        std::vector<unsigned short> alleles = {0, 1};
        std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> chromosomes;
        chromosomes["chr2"] = {std::make_shared<BiallelicUniqueKmers>(99, alleles)};
        std::map<std::string, Graph> none;
        std::vector<SampleCounts> samples(1);
        ProbabilityTable probs(1, 160, 80, 0.01L);
        CHECK(what_of([&] { genotype_cohort_sampled_record_lines(chromosomes, none, samples, 7, true, 10, 25000.0L, &probs); }).find("no graph of chr2") != std::string::npos);
        CHECK(genotype_cohort_sampled_record_lines(chromosomes, none, {}, 7, true, 10, 25000.0L, &probs).empty());
    });
}

// one sample's lines of one chromosome against the '\n'-joined genotypes_records of its text; answers the records compared
static size_t compare(const Graph& graph, const RecordLines& l, const RecordText& t, size_t* bytes, size_t* no_call) {
    const std::vector<std::string> want = graph.genotypes_records(t);
    const size_t R = want.size();
    CHECK(l.off.size() == R + 1 && l.off[0] == 0 && l.off.back() == l.bytes.size());
    if (l.off.size() != R + 1) return 0;
    std::string joined;
    size_t ok = 0;
    for (size_t r = 0; r < R; ++r) {
        const bool same = l.off[r] == joined.size() && l.off[r + 1] >= l.off[r] && l.bytes.compare(l.off[r], l.off[r + 1] - l.off[r], want[r] + '\n') == 0;
        if (!same && g_failed <= 20) std::printf("    record %zu:\n      %s      %s\n", r, l.bytes.substr(l.off[r], l.off[r + 1] - l.off[r]).c_str(), want[r].c_str());
        ok += same;
        joined += want[r] + '\n';
        *no_call += want[r].find("\t.:.:") != std::string::npos;
    }
    CHECK(ok == R && l.bytes == joined);
    *bytes += l.bytes.size();
    return R;
}

static void lines_against_text(const std::function<UniqueKmersMap()>& fresh, const std::map<std::string, Graph>& graphs, const std::vector<SampleCounts>& counts,
                               ProbabilityTable& probs, size_t panel_size, size_t records) {
    run("genotype_cohort_sampled_record_lines = the joined Graph::genotypes_records(genotype_cohort_sampled_record_text); the written file", [&] {
        size_t compared = 0, bytes = 0, no_call = 0, uk_differs = 0;
        for (const bool ignore_imputed : {false, true}) {
            UniqueKmersMap m = fresh(), other = fresh();
            std::vector<std::map<std::string, SampledPaths>> want_picks, got_picks;
            const auto text = genotype_cohort_sampled_record_text(other.unique_kmers, graphs, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0,
                                                                  ignore_imputed, &want_picks);
            const auto lines = genotype_cohort_sampled_record_lines(m.unique_kmers, graphs, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0,
                                                                    ignore_imputed, &got_picks);
            CHECK(text.size() == counts.size() && lines.size() == counts.size() && got_picks.size() == want_picks.size());
            for (size_t s = 0; s < text.size() && s < lines.size(); ++s) {
                CHECK(lines[s].size() == graphs.size());
                for (const auto& kv : text[s]) {
                    const auto found = lines[s].find(kv.first);
                    CHECK(found != lines[s].end());
                    if (found == lines[s].end()) continue;
                    const Graph& graph = graphs.at(kv.first);
                    compared += compare(graph, found->second, kv.second, &bytes, &no_call);
                    uk_differs += s > 0 && kv.second.unique_kmers != text[0].at(kv.first).unique_kmers;
                    if (s < got_picks.size() && s < want_picks.size()) CHECK(got_picks[s].count(kv.first) == want_picks[s].count(kv.first));
                    if (ignore_imputed) continue;
                    // the file: the header, then the body in one write; read back equal
                    const std::string path = "test_sampled_record_lines_host." + kv.first + ".tmp.vcf", name = "sample" + std::to_string(s);
                    graph.write_genotypes(path, kv.second, true, name);
                    const std::string want = file_bytes(path);
                    graph.write_genotypes(path, found->second, true, std::vector<std::string>{name});
                    const std::string got = file_bytes(path);
                    std::remove(path.c_str());
                    CHECK(got == want && got.size() > found->second.bytes.size());
                    CHECK(got.size() >= found->second.bytes.size() && got.compare(got.size() - found->second.bytes.size(), std::string::npos, found->second.bytes) == 0);
                }
            }
        }
        CHECK(compared == 2 * counts.size() * records && bytes > 20 * compared);
        std::printf("  %zu lines compared, %zu bytes, %zu lines without a call, UK differs between samples on %zu chromosome(s)\n", compared, bytes, no_call, uk_differs);
    });
}

int main(int argc, char** argv) {
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (mode == "cpu" && argc >= 3) {
        cpu_tests(argv[2]);
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (mode == "counted" && argc >= 8) {
        const std::string archive = argv[2], graph_archive = argv[3];
        ProbabilityTable probs((unsigned)std::atoi(argv[4]), (unsigned)std::atoi(argv[5]), (unsigned)std::atoi(argv[6]), 0.01L);
        const size_t panel_size = (size_t)std::atoi(argv[7]);
        auto fresh = [&] { return load_unique_kmers_map(archive); };
        const UniqueKmersMap index = fresh();
        std::map<std::string, Graph> graphs;
        size_t records = 0;
        for (const auto& kv : index.unique_kmers) {
            graphs[kv.first] = Graph::load(graph_archive);
            records += graphs[kv.first].record_plan().nr_of_records();
        }
        const SampleCounts one = SampleCounts::of(index.unique_kmers);
        lines_against_text(fresh, graphs, {one, one}, probs, panel_size, records);
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (mode != "gpu" || argc < 5) {
        std::printf("usage: test_sampled_record_lines_host cpu <graph> | counted <archive> <graph> <cov min> <cov max> <count max> <panel size> | gpu <index prefix> <reads 1> <reads 2>\n");
        return 2;
    }
    const std::string prefix = argv[2];
    const std::vector<std::string> reads = {argv[3], argv[4]};
    const std::vector<size_t> coverage = {20, 17};
    auto fresh = [&] { return load_unique_kmers_map(prefix + "_UniqueKmersMap.cereal"); };
    const UniqueKmersMap index = fresh();
    std::map<std::string, Graph> graphs;
    size_t merged = 0, records = 0;
    for (const auto& kv : index.unique_kmers) {
        graphs[kv.first] = Graph::load(prefix + "_" + kv.first + "_Graph.cereal");
        const Graph& g = graphs[kv.first];
        for (size_t v = 0; v < g.size(); ++v) merged += g.get_variant(v).nr_of_records() >= 2;
        records += g.record_plan().nr_of_records();
    }
    std::vector<SampleCounts> counts;
    {
        UniqueKmersMap m = fresh();
        DeviceKmerCounter dev(m.kmersize);
        DeviceCountPlan plan(dev, m, prefix, true);
        for (size_t s = 0; s < 2; ++s) {
            dev.reset_counts();
            dev.count(reads[s]);
            counts.push_back(plan.fill(coverage[s]));
        }
    }
    ProbabilityTable probs(1, 160, 80, 0.01L);
    CHECK(merged >= 1 && records > 100);   // the input holds what this test is about
    lines_against_text(fresh, graphs, counts, probs, 7, records);
    run("genotype_cohort_sampled_reads_record_lines = genotype_cohort_sampled_record_lines on the counts of the same reads; batch 1 and 2", [&] {
        for (const bool ignore_imputed : {false, true}) {
            UniqueKmersMap m = fresh(), other = fresh();
            const auto want = genotype_cohort_sampled_record_lines(other.unique_kmers, graphs, counts, 7, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
            const auto got = genotype_cohort_sampled_reads_record_lines(m, graphs, prefix, reads, coverage, 7, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0,
                                                                        ignore_imputed ? 1 : 2, ignore_imputed);
            CHECK(got.size() == want.size() && got.size() == 2);
            for (size_t s = 0; s < want.size() && s < got.size(); ++s)
                for (const auto& kv : want[s]) {
                    const auto found = got[s].find(kv.first);
                    CHECK(found != got[s].end());
                    if (found == got[s].end()) continue;
                    CHECK(found->second.bytes == kv.second.bytes && found->second.off == kv.second.off && !kv.second.bytes.empty());
                }
        }
    });
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
