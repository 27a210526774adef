// test_record_text_host.cpp — the VCF lines with the sample column arriving as bytes from the device
// (pangenie_amd/host/graph_io.hpp: RecordText, Graph::genotypes_records(RecordText), genotype_cohort_record_text,
// genotype_cohort_sampled_record_text; kmer_counts.hpp: genotype_cohort_sampled_reads_record_text) against the lines of their _record_fields siblings' output through the existing
// overload.  Text for text, whole lines, with and without ignore_imputed.
//   test_record_text_host cpu
//       the splice on a hand-made RecordText and its refusals; record_field_text; no device
//   test_record_text_host counted <UniqueKmersMap archive with read counts> <Graph archive> <cov min> <cov max> <count max> <panel size> [<expected VCF>]
//       one sample, the counts the archive holds (the reference's region fixture; the demo's counted index): both routes;
//       with an expected VCF, its records' sample columns are the text's
//   test_record_text_host gpu <index prefix> <reads of sample 1> <reads of sample 2>
//       two samples on the simulated pangenome of the other host tests (merged bubbles, alleles of undefined sequence)
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
static pg_gl gl(int mant, int exp10) { pg_gl g; g.mant = (int16_t)mant; g.exp10 = (int16_t)exp10; return g; }
static GenotypeCall call(int a, int b, size_t gq) { GenotypeCall c; c.allele_1 = a; c.allele_2 = b; c.quality = gq; return c; }
static std::string field_of(const std::string& line) { return line.substr(line.rfind('\t') + 1); }

static void cpu_tests() {
    run("Graph::genotypes_records(RecordText): the splice of hand-made bytes, record_field_text, the refusals", [] {
        Variant snp = Variant::from_parts("chr2", 99, "AAAA", "CCCC", {{"C", "G"}}, {}, {{0}, {1}}, {0, 1, 1, 0}, true);
        Variant lone = Variant::from_parts("chr2", 199, "AAAA", "CCCC", {{"C", "CNN"}}, {}, {{0}, {1}}, {0, 1, 1, 0}, true);   // ALT undefined: one defined allele
        Graph graph = Graph::from_parts("chr2", 4, false, {snp}, {{"id-G"}});
        RecordFields f;
        f.calls = {call(0, 0, 4)};
        f.gl = {gl(-1761, -1), gl(-4771, -1), gl(0, PG_GL_NEG_INF)};
        f.gl_off = {0, 3};
        const std::vector<std::string> want = graph.genotypes_records(f, {7}, {14});
        CHECK(record_field_text(f, 0, 7, false) == "0/0:4:-0.1761,-0.4771,-inf:7" && record_field_text(f, 0, 7, true) == ".:.:-0.1761,-0.4771,-inf:7");
        RecordText t;
        t.bytes = "0/0:4:-0.1761,-0.4771,-inf:7";
        t.off = {0, t.bytes.size()};
        t.unique_kmers = {14};
        const std::vector<std::string> got = graph.genotypes_records(t);
        CHECK(got.size() == 1 && want.size() == 1 && got[0] == want[0]);
        if (got.size() == 1 && want.size() == 1 && got[0] != want[0]) std::printf("    %s\n    %s\n", got[0].c_str(), want[0].c_str());
        // the bytes are spliced in as they are, UK comes from the text's own array
        t.bytes = ".:.:-0.1761,-0.4771,-inf:7";
        t.off = {0, t.bytes.size()};
        t.unique_kmers = {0};
        CHECK(graph.genotypes_records(t)[0] == graph.genotypes_records(f, {7}, {0}, true)[0]);
        // refusals: an empty record that somebody should have finished, offsets that do not fit, another number of bubbles
        t.off = {0, 0};
        CHECK(what_of([&] { graph.genotypes_records(t); }).find("left to the host") != std::string::npos);
        t.off = {0, 100};
        CHECK(what_of([&] { graph.genotypes_records(t); }).find("does not fit") != std::string::npos);
        t.off = {0};
        CHECK(what_of([&] { graph.genotypes_records(t); }).find("does not fit") != std::string::npos);
        t.off = {0, t.bytes.size()};
        t.unique_kmers = {0, 0};
        CHECK(what_of([&] { graph.genotypes_records(t); }).find("number of variants") != std::string::npos);
        // a record with fewer than two defined alleles has no text: the error of the existing overloads
        Graph lonely = Graph::from_parts("chr2", 4, false, {lone}, {{}});
        RecordFields one;
        one.calls = {call(0, 0, 10000)};
        one.gl = {gl(0, 0)};
        one.gl_off = {0, 1};
        RecordText none;
        none.off = {0, 0};
        none.unique_kmers = {14};
        const std::string theirs = what_of([&] { lonely.genotypes_records(one, {7}, {14}); }), ours = what_of([&] { lonely.genotypes_records(none); });
        CHECK(theirs.find("too few likelihoods (1)") != std::string::npos && ours == theirs);
        CHECK(what_of([&] { record_field_text(one, 0, 7, false); }) == theirs);
        // write_genotypes: header and records
        const std::string path = "test_record_text_host.tmp.vcf";
        t.unique_kmers = {0};
        graph.write_genotypes(path, t, true, "sample");
        std::ifstream in(path);
        std::string line, last;
        size_t n = 0;
        while (std::getline(in, line)) { last = line; ++n; }
        std::remove(path.c_str());
        CHECK(n == Graph::genotypes_header("sample").size() + 1 && last == graph.genotypes_records(t)[0]);
    });
    run("genotype_cohort[_sampled]_record_text refuse a missing graph before any job, and do nothing without chromosomes or samples", [] {
        std::vector<unsigned short> alleles = {0, 1};
        std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> chromosomes, empty;
        chromosomes["chr2"] = {std::make_shared<BiallelicUniqueKmers>(99, alleles)};
        std::map<std::string, Graph> none;
        std::vector<SampleCounts> samples(1);
        ProbabilityTable probs(1, 160, 80, 0.01L);
        CHECK(what_of([&] { genotype_cohort_record_text(chromosomes, none, samples, &probs); }).find("no graph of chr2") != std::string::npos);
        CHECK(what_of([&] { genotype_cohort_sampled_record_text(chromosomes, none, samples, 7, true, 10, 25000.0L, &probs); }).find("no graph of chr2") != std::string::npos);
        CHECK(genotype_cohort_record_text(empty, none, samples, &probs).size() == 1);
        CHECK(genotype_cohort_sampled_record_text(chromosomes, none, {}, 7, true, 10, 25000.0L, &probs).empty());
    });
}

struct Stats { size_t compared = 0, no_call = 0, bytes = 0; };

// the lines of the text against the lines of the sibling's fields through the existing overload
static void compare(const Graph& graph, const RecordText& t, const RecordFields& f, const std::vector<unsigned short>& cov, const std::vector<unsigned short>& uk,
                    bool ignore_imputed, Stats* st, std::vector<std::string>* fields_out = nullptr) {
    const std::vector<std::string> lines = graph.genotypes_records(f, cov, uk, ignore_imputed);
    const std::vector<std::string> ours = graph.genotypes_records(t);
    CHECK(ours.size() == lines.size() && t.off.size() == lines.size() + 1 && t.unique_kmers == uk);
    for (size_t r = 0; r < lines.size() && r < ours.size(); ++r) {
        CHECK(ours[r] == lines[r]);
        if (ours[r] != lines[r] && g_failed <= 20) std::printf("    record %zu:\n      %s\n      %s\n", r, ours[r].c_str(), lines[r].c_str());
        st->compared += 1;
        st->no_call += lines[r].find("\t.:.:") != std::string::npos;
        if (fields_out) fields_out->push_back(field_of(ours[r]));
    }
    st->bytes += t.bytes.size();
}

// both routes on `counts` over the index `fresh()` loads (a UniqueKmersMap copies its objects by pointer: every route loads its own)
static void both_routes(const std::function<UniqueKmersMap()>& fresh, const std::map<std::string, Graph>& graphs, const std::vector<SampleCounts>& counts,
                        ProbabilityTable& probs, size_t panel_size, size_t records, std::vector<std::string>* demo_fields) {
    run("Graph::genotypes_records(genotype_cohort_record_text) = Graph::genotypes_records(genotype_cohort_record_fields)", [&] {
        UniqueKmersMap m = fresh(), other = fresh(), third = fresh();
        auto results = genotype_cohort(third.unique_kmers, counts, &probs, 1.26, false, 0.00001L, 0);   // (KC and UK as the sibling's caller has them)
        Stats st;
        for (const bool ignore_imputed : {false, true}) {
            const auto want = genotype_cohort_record_fields(other.unique_kmers, graphs, counts, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
            const auto got = genotype_cohort_record_text(m.unique_kmers, graphs, counts, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
            CHECK(got.size() == want.size() && got.size() == counts.size());
            for (size_t s = 0; s < want.size() && s < got.size(); ++s)
                for (const auto& kv : want[s]) {
                    const auto found = got[s].find(kv.first);
                    CHECK(found != got[s].end());
                    if (found == got[s].end()) continue;
                    std::vector<unsigned short> cov, uk;
                    for (const GenotypingResult& r : results[s].at(kv.first)) { cov.push_back(r.coverage()); uk.push_back(r.nr_unique_kmers()); }
                    compare(graphs.at(kv.first), found->second, kv.second, cov, uk, ignore_imputed, &st, !ignore_imputed && s == 0 ? demo_fields : nullptr);
                }
        }
        CHECK(st.compared == 2 * counts.size() * records && st.bytes > 20 * st.compared);
        std::printf("  %zu lines compared, %zu bytes of text, %zu lines without a call\n", st.compared, st.bytes, st.no_call);
    });
    if (panel_size == 0) return;
    run("Graph::genotypes_records(genotype_cohort_sampled_record_text) = Graph::genotypes_records(genotype_cohort_sampled_record_fields)", [&] {
        UniqueKmersMap m = fresh(), other = fresh();
        Stats st;
        for (const bool ignore_imputed : {false, true}) {
            std::vector<std::map<std::string, SampledPaths>> want_picks, got_picks;
            const auto want = genotype_cohort_sampled_record_fields(other.unique_kmers, graphs, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L,
                                                                    0, ignore_imputed, &want_picks);
            const auto got = genotype_cohort_sampled_record_text(m.unique_kmers, graphs, counts, panel_size, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0,
                                                                 ignore_imputed, &got_picks);
            CHECK(got.size() == want.size() && got.size() == counts.size() && got_picks.size() == want_picks.size());
            for (size_t s = 0; s < want.size() && s < got.size(); ++s)
                for (const auto& kv : want[s]) {
                    const auto found = got[s].find(kv.first);
                    CHECK(found != got[s].end());
                    if (found == got[s].end()) continue;
                    compare(graphs.at(kv.first), found->second, kv.second.fields, kv.second.coverage, kv.second.unique_kmers, ignore_imputed, &st);
                    CHECK(s < got_picks.size() && got_picks[s].count(kv.first) && got_picks[s].at(kv.first).sampled_paths == want_picks[s].at(kv.first).sampled_paths);
                }
        }
        CHECK(st.compared == 2 * counts.size() * records && st.bytes > 20 * st.compared);
        std::printf("  sampled to %zu + 1 paths: %zu lines compared, %zu bytes of text, %zu lines without a call\n", panel_size, st.compared, st.bytes, st.no_call);
    });
}

int main(int argc, char** argv) {
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (mode == "cpu") {
        cpu_tests();
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
        const std::vector<SampleCounts> counts = {SampleCounts::of(index.unique_kmers)};
        std::vector<std::string> fields;
        both_routes(fresh, graphs, counts, probs, panel_size, records, &fields);
        if (argc >= 9)
            run("the sample columns are those of the expected VCF", [&] {
                std::ifstream in(argv[8]);
                std::string line;
                std::vector<std::string> want;
                while (std::getline(in, line))
                    if (!line.empty() && line[0] != '#') want.push_back(field_of(line));
                CHECK(want.size() == records && fields == want);
                for (size_t r = 0; r < want.size() && r < fields.size(); ++r)
                    if (fields[r] != want[r]) std::printf("    record %zu: %s / %s\n", r, fields[r].c_str(), want[r].c_str());
            });
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (mode != "gpu" || argc < 5) {
        std::printf("usage: test_record_text_host cpu | counted <archive> <graph> <cov min> <cov max> <count max> <panel size> [<expected VCF>] | gpu <index prefix> <reads 1> <reads 2>\n");
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
    both_routes(fresh, graphs, counts, probs, 7, records, nullptr);
    run("Graph::genotypes_records(genotype_cohort_sampled_reads_record_text) = Graph::genotypes_records(genotype_cohort_sampled_reads_record_fields); batch 1 and 2", [&] {
        UniqueKmersMap m = fresh(), other = fresh();
        Stats st;
        for (const bool ignore_imputed : {false, true}) {   // (KC comes from the coverage the count plan wrote on the device)
            const auto want = genotype_cohort_sampled_reads_record_fields(other, graphs, prefix, reads, coverage, 7, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L,
                                                                          0, 2, ignore_imputed);
            const auto got = genotype_cohort_sampled_reads_record_text(m, graphs, prefix, reads, coverage, 7, true, 10, 25000.0L, &probs, 1.26, false, 0.00001L, 0,
                                                                       ignore_imputed ? 1 : 2, ignore_imputed);
            CHECK(got.size() == want.size() && got.size() == 2);
            for (size_t s = 0; s < want.size() && s < got.size(); ++s)
                for (const auto& kv : want[s]) {
                    const auto found = got[s].find(kv.first);
                    CHECK(found != got[s].end());
                    if (found != got[s].end()) compare(graphs.at(kv.first), found->second, kv.second.fields, kv.second.coverage, kv.second.unique_kmers, ignore_imputed, &st);
                }
        }
        CHECK(st.compared == 4 * records);
        std::printf("  from reads: %zu lines compared, %zu bytes of text\n", st.compared, st.bytes);
    });
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
