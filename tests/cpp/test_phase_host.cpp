// test_phase_host.cpp — the phasing VCF with its `GT:KC` column formed on the device (pangenie_amd/host/graph_io.hpp:
// phase_cohort_record_text, phase_cohort_record_lines, Graph::phasing_fixed_columns, Graph::phasing_header(samples),
// Graph::phasing_records(RecordText), Graph::write_phasing(RecordLines)) against the host's route: an
// HMM(..., false, true, ..., only_paths) per sample and Graph::phasing_records over its results.  Line for line.
//   test_phase_host cpu <Graph archive>
//       the fixed columns are what every line of phasing_records begins with; the multi-sample header; the file; the check
//       for a REF of undefined sequence; the drivers' refusals; no device
//   test_phase_host counted <UniqueKmersMap archive with read counts> <Graph archive> <cov min> <cov max> <count max> <paths>
//       the counts the archive holds as one sample and as two, over every (n_paths / paths)-th path; then the same with a
//       graph whose ALT alleles are all of undefined sequence (`.` on the device route) and with one whose first REF is: the
//       host route inside the drivers
//   test_phase_host vcf <counted archive> <Graph archive> <cov min> <cov max> <count max> <out.vcf>
//       the phasing run of one sample over all paths through the device route, written by write_phasing(RecordLines)
#include <cstdio>
#include <cstdlib>
#include <fstream>
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
static std::string what_of(const std::function<void()>& f) {
    try { f(); } catch (const std::exception& e) { return e.what(); }
    return "";
}
static std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) {
        const size_t next = s.find(sep, at);
        out.push_back(s.substr(at, next == std::string::npos ? std::string::npos : next - at));
        if (next == std::string::npos) break;
        at = next + 1;
    }
    return out;
}
static std::vector<std::string> lines_of_file(const std::string& path) {
    std::ifstream in(path);
    std::vector<std::string> lines;
    std::string line;
    while (std::getline(in, line)) lines.push_back(line);
    return lines;
}

// a hand-made phased text of R records: sample s, record r
static RecordText made_text(size_t R, size_t s, const std::vector<unsigned short>& uk) {
    RecordText t;
    t.off.assign(1, 0);
    for (size_t r = 0; r < R; ++r) {
        t.bytes += (r % 3 == 2 ? "." : std::to_string(s)) + "|" + std::to_string(r % 3) + ":" + std::to_string((r * 7 + s) % 60);
        t.off.push_back(t.bytes.size());
    }
    t.unique_kmers = uk;
    return t;
}

// the graph of the fixture with the REF of its first record (`ref`), or every ALT of every record (`alts`), replaced by a
// sequence that holds an N
static Graph with_undefined(const Graph& graph, bool ref, bool alts) {
    const RecordPlan plan = graph.record_plan();
    std::vector<Variant> variants;
    for (size_t i = 0; i < graph.size(); ++i) {
        const Variant& v = graph.get_variant(i);
        if (v.nr_of_records() != 1) throw std::runtime_error("with_undefined_reference: a bubble of one record each is expected");
        std::vector<std::string> alleles = v.records(nullptr).at(0).alleles;
        if (ref && i == 0) alleles[0] = std::string(alleles[0].size(), 'N');
        for (size_t a = 1; alts && a < alleles.size(); ++a) alleles[a] = std::string(alleles[a].empty() ? 1 : alleles[a].size(), 'N');
        std::vector<std::vector<unsigned short>> combinations;
        for (size_t a = 0; a < v.nr_of_alleles(); ++a) combinations.push_back({plan.map.at(plan.map_off.at(i) + a)});
        std::vector<unsigned short> paths;
        for (size_t p = 0; p < v.nr_of_paths(); ++p) paths.push_back(v.get_allele_on_path(p));
        variants.push_back(Variant::from_parts(v.get_chromosome(), v.get_start_position(), "", "", {alleles}, {}, combinations, paths, false));
    }
    // (the ids name ALT alleles: a graph without defined ALT alleles has none)
    return Graph::from_parts(graph.get_chromosome(), graph.get_kmer_size(), graph.reference_added(), variants,
                             alts ? std::vector<std::vector<std::string>>(graph.variant_ids().size()) : graph.variant_ids());
}

static void cpu_tests(const std::string& graph_archive) {
    const Graph graph = Graph::load(graph_archive);
    const size_t R = graph.record_plan().nr_of_records();
    std::vector<unsigned short> uk(graph.size());
    for (size_t v = 0; v < uk.size(); ++v) uk[v] = (unsigned short)((v * 13 + 5) % 301);
    run("Graph::phasing_fixed_columns: what every line of phasing_records(RecordText) begins with, and of phasing_records(results)", [&] {
        const std::vector<std::string> fixed = graph.phasing_fixed_columns(uk), genotyped = graph.genotypes_fixed_columns(uk);
        const RecordText t = made_text(R, 1, uk);
        const std::vector<std::string> lines = graph.phasing_records(t);
        CHECK(R >= 2 && fixed.size() == R && lines.size() == R && genotyped.size() == R);
        std::vector<GenotypingResult> results(graph.size());
        for (size_t v = 0; v < results.size(); ++v) { results[v].set_unique_kmers(uk[v]); results[v].set_coverage(9); }
        const std::vector<std::string> hosts = graph.phasing_records(results);
        for (size_t r = 0; r < R && r < fixed.size() && r < lines.size(); ++r) {
            CHECK(lines[r] == fixed[r] + '\t' + t.bytes.substr(t.off[r], t.off[r + 1] - t.off[r]));
            CHECK(hosts[r].rfind(fixed[r] + '\t', 0) == 0);
            const std::vector<std::string> cols = split(fixed[r], '\t'), other = split(genotyped[r], '\t');
            CHECK(cols.size() == 9 && cols[8] == "GT:KC" && cols[7].find(";UK=") != std::string::npos && other.size() == 9);
            for (size_t k = 0; k < 8 && k < cols.size() && k < other.size(); ++k) CHECK(cols[k] == other[k]);   // (one fixed_columns_of)
        }
        CHECK(what_of([&] { graph.phasing_fixed_columns(std::vector<unsigned short>(uk.size() + 1, 0)); }).find("number of variants") != std::string::npos);
        RecordText hole = t;
        hole.off[1] = hole.off[0];
        CHECK(what_of([&] { graph.phasing_records(hole); }).find("a record's text is empty") != std::string::npos);
        RecordText brief = t;
        brief.off.pop_back();
        CHECK(what_of([&] { graph.phasing_records(brief); }).find("does not fit") != std::string::npos);
    });
    run("Graph::phasing_header(samples): the names joined by tabs", [&] {
        const std::vector<std::string> one = Graph::phasing_header("a", "20240101"), three = Graph::phasing_header(std::vector<std::string>{"a", "b", "c"}, "20240101");
        CHECK(one.size() == 10 && one.size() == three.size() && three.back() == one.back() + "\tb\tc");
        for (size_t i = 0; i + 1 < one.size() && i + 1 < three.size(); ++i) CHECK(one[i] == three[i]);
        CHECK(Graph::phasing_header(std::vector<std::string>{"a"}, "20240101") == one);
    });
    run("Graph::write_phasing(RecordLines): header and body, appended without a header, the refusals", [&] {
        const std::vector<std::string> fixed = graph.phasing_fixed_columns(uk);
        const RecordText t0 = made_text(R, 0, uk), t1 = made_text(R, 1, uk);
        RecordLines none;
        none.off.assign(R + 1, 0);
        const RecordLines lines = compose_record_lines(fixed, {&t0, &t1}, none);
        const std::string path = "test_phase_host.tmp.vcf";
        graph.write_phasing(path, lines, true, {"s0", "s1"});
        std::vector<std::string> got = lines_of_file(path);
        const size_t H = Graph::phasing_header("x").size();
        CHECK(got.size() == H + R && got[H - 1] == Graph::phasing_header(std::vector<std::string>{"s0", "s1"}).back());
        const std::vector<std::string> a = graph.phasing_records(t0), b = graph.phasing_records(t1);
        size_t ok = 0;
        for (size_t r = 0; r < R && H + r < got.size(); ++r) ok += got[H + r] == a[r] + '\t' + split(b[r], '\t').at(9);
        CHECK(ok == R);
        graph.write_phasing(path, lines, false, {"s0", "s1"});
        got = lines_of_file(path);
        CHECK(got.size() == H + 2 * R && got[H + R] == got[H]);
        std::remove(path.c_str());
        RecordLines bad = lines;
        bad.off[1] = bad.off[0];
        CHECK(what_of([&] { graph.write_phasing(path, bad, true, {"s0", "s1"}); }).find("empty or unfinished") != std::string::npos);
        bad = lines;
        bad.off.pop_back();
        CHECK(what_of([&] { graph.write_phasing(path, bad, true, {"s0", "s1"}); }).find("do not fit") != std::string::npos);
        CHECK(lines_of_file(path).empty());   // (refused before the file is touched)
    });
    run("Graph::has_undefined_reference_allele: the plan calls REF defined, the host prints . for it", [&] {
        CHECK(!graph.has_undefined_reference_allele());
        const Graph other = with_undefined(graph, true, false);
        CHECK(other.has_undefined_reference_allele() && other.size() == graph.size());
        CHECK(other.record_plan().vcf_index == graph.record_plan().vcf_index);   // (REF stays index 0 in the plan)
        std::vector<GenotypingResult> results(other.size());
        results[0].add_first_haplotype_allele(0); results[0].add_second_haplotype_allele(1);
        const std::vector<std::string> lines = other.phasing_records(results);
        CHECK(!lines.empty() && split(lines[0], '\t').back() == ".|0:0");   // (no likelihoods: the defined ALT comes out as 0)
    });
    run("the phasing drivers refuse a missing graph before any job, and do nothing without chromosomes", [] {
        std::vector<unsigned short> alleles = {0, 1};
        std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> chromosomes, empty;
        chromosomes["chr2"] = {std::make_shared<BiallelicUniqueKmers>(99, alleles)};
        std::map<std::string, Graph> none;
        std::vector<SampleCounts> samples(1);
        ProbabilityTable probs(1, 160, 80, 0.01L);
        CHECK(what_of([&] { phase_cohort_record_text(chromosomes, none, samples, &probs); }).find("phase_cohort_record_text: no graph of chr2") != std::string::npos);
        CHECK(what_of([&] { phase_cohort_record_lines(chromosomes, none, samples, &probs); }).find("phase_cohort_record_lines: no graph of chr2") != std::string::npos);
        CHECK(phase_cohort_record_text(empty, none, samples, &probs).size() == 1 && phase_cohort_record_lines(empty, none, samples, &probs).empty());
    });
}

// the host's route: per sample an HMM that runs the phasing alone over `only_paths`, its results printed by phasing_records
static std::vector<std::string> host_lines(UniqueKmersMap& m, const std::string& chromosome, const Graph& graph, ProbabilityTable& probs,
                                           std::vector<unsigned short>& only_paths, bool ignore_imputed) {
    HMM viterbi(&m.unique_kmers.at(chromosome), &probs, false, true, 1.26, false, 0.00001L, &only_paths, false);
    return graph.phasing_records(viterbi.get_genotyping_result(), ignore_imputed);
}

static void drivers_against_the_host(const std::function<UniqueKmersMap()>& fresh, const std::map<std::string, Graph>& graphs, size_t S, ProbabilityTable& probs,
                                     std::vector<unsigned short>& only_paths, size_t records, const char* which, bool dots_expected) {
    const std::string name = std::string("phase_cohort_record_text / _lines, ") + std::to_string(S) + " sample(s), " + which + ": the lines of Graph::phasing_records over an HMM's results";
    run(name.c_str(), [&] {
        size_t compared = 0, dots = 0, no_call = 0;
        for (const bool ignore_imputed : {false, true}) {
            UniqueKmersMap a = fresh(), b = fresh(), c = fresh();
            const std::vector<SampleCounts> counts(S, SampleCounts::of(a.unique_kmers));
            const auto text = phase_cohort_record_text(a.unique_kmers, graphs, counts, &probs, &only_paths, 1.26, false, 0.00001L, 0, ignore_imputed);
            const auto lines = phase_cohort_record_lines(b.unique_kmers, graphs, counts, &probs, &only_paths, 1.26, false, 0.00001L, 0, ignore_imputed);
            CHECK(text.size() == S && lines.size() == graphs.size());
            for (const auto& kv : lines) {
                const Graph& graph = graphs.at(kv.first);
                const std::vector<std::string> want = host_lines(c, kv.first, graph, probs, only_paths, ignore_imputed);
                const size_t R = want.size();
                for (size_t s = 0; s < S; ++s) {   // the single-sample lines, text for text
                    const std::vector<std::string> got = graph.phasing_records(text[s].at(kv.first));
                    CHECK(got == want);
                    if (got != want && g_failed <= 20)
                        for (size_t r = 0; r < R && r < got.size(); ++r)
                            if (got[r] != want[r]) { std::printf("    %s record %zu:\n      %s\n      %s\n", kv.first.c_str(), r, got[r].c_str(), want[r].c_str()); break; }
                }
                const RecordLines& l = kv.second;
                CHECK(l.off.size() == R + 1 && l.off[0] == 0 && l.off.back() == l.bytes.size());
                if (l.off.size() != R + 1) continue;
                for (size_t r = 0; r < R; ++r) {   // the multi-sample line: the host's line, its last column once per sample
                    std::string line = want[r];
                    const std::string column = split(want[r], '\t').back();
                    for (size_t s = 1; s < S; ++s) line += '\t' + column;
                    CHECK(l.bytes.substr(l.off[r], l.off[r + 1] - l.off[r]) == line + '\n');
                    dots += column.find('.') != std::string::npos;
                    no_call += column.rfind("./.", 0) == 0;
                    compared += 1;
                }
            }
        }
        CHECK(compared == 2 * records);
        // the fixture's own haplotypes over these paths are on defined alleles, and its bubbles have k-mers (no ./.): a `.` is
        // certain only where the graph was given undefined alleles the haplotypes are on
        if (dots_expected) CHECK(dots > 0);
        std::printf("  %zu lines of %zu sample(s) compared, %zu columns with a `.`, %zu of them ./.\n", compared, S, dots, no_call);
    });
}

int main(int argc, char** argv) {
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (mode == "cpu" && argc >= 3) {
        cpu_tests(argv[2]);
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if ((mode == "counted" && argc >= 8) || (mode == "vcf" && argc >= 8)) {
        const std::string archive = argv[2], graph_archive = argv[3];
        ProbabilityTable probs((unsigned)std::atoi(argv[4]), (unsigned)std::atoi(argv[5]), (unsigned)std::atoi(argv[6]), 0.01L);
        auto fresh = [&] { return load_unique_kmers_map(archive); };
        const UniqueKmersMap index = fresh();
        std::map<std::string, Graph> graphs, undefined_ref;
        size_t records = 0, n_paths = 0;
        for (const auto& kv : index.unique_kmers) {
            graphs[kv.first] = Graph::load(graph_archive);
            records += graphs[kv.first].record_plan().nr_of_records();
            if (!kv.second.empty()) n_paths = kv.second[0]->get_nr_paths();
        }
        if (mode == "vcf") {   // one sample over all paths (at most 30 in the demo), the file by write_phasing(RecordLines)
            UniqueKmersMap m = fresh();
            const std::vector<SampleCounts> counts(1, SampleCounts::of(m.unique_kmers));
            const auto lines = phase_cohort_record_lines(m.unique_kmers, graphs, counts, &probs, nullptr, 1.26, false, 0.00001L, 0, false);
            std::remove(argv[7]);
            bool header = true;
            for (const auto& kv : lines) { graphs.at(kv.first).write_phasing(argv[7], kv.second, header, {"sample"}); header = false; }
            return 0;
        }
        const size_t wanted = (size_t)std::atoi(argv[7]);
        std::vector<unsigned short> only_paths;
        for (size_t p = 0; p < wanted && p * (n_paths / wanted) < n_paths; ++p) only_paths.push_back((unsigned short)(p * (n_paths / wanted)));
        CHECK(only_paths.size() == wanted && wanted <= 64 && records >= 2);
        drivers_against_the_host(fresh, graphs, 1, probs, only_paths, records, "the fixture's graph", false);
        drivers_against_the_host(fresh, graphs, 2, probs, only_paths, records, "the fixture's graph", false);
        std::map<std::string, Graph> undefined_alts;   // still the device route: REF is defined, every haplotype off REF prints .
        for (const auto& kv : graphs) undefined_alts[kv.first] = with_undefined(kv.second, false, true);
        drivers_against_the_host(fresh, undefined_alts, 2, probs, only_paths, records, "every ALT of undefined sequence (the device route)", true);
        for (const auto& kv : graphs) undefined_ref[kv.first] = with_undefined(kv.second, true, false);
        drivers_against_the_host(fresh, undefined_ref, 2, probs, only_paths, records, "a REF of undefined sequence (the host route)", true);
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    std::printf("usage: test_phase_host cpu <graph> | counted <archive> <graph> <cov min> <cov max> <count max> <paths> | vcf <archive> <graph> <cov min> <cov max> <count max> <out.vcf>\n");
    return 2;
}
