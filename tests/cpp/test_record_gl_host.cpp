// test_record_gl_host.cpp — the VCF lines from the device's record fields (pangenie_amd/host/graph_io.hpp:
// genotype_cohort_record_fields, Graph::genotypes_records(const RecordFields&, ...)) against the lines of the route they spare:
// genotype_cohort, GenotypingResult::normalize, Graph::genotypes_records on the results.  Text for text, whole lines, with
// and without ignore_imputed.
//   test_record_gl_host gpu <index prefix> <reads of sample 1> <reads of sample 2>
//   test_record_gl_host cpu          the overload on hand-made fields, and its refusals; no device
// <index prefix>: as for tests/cpp/test_record_calls_host.cpp (merged bubbles, alleles of undefined sequence).
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

static pg_gl gl(int mant, int exp10) { pg_gl g; g.mant = (int16_t)mant; g.exp10 = (int16_t)exp10; return g; }
static GenotypeCall call(int a, int b, size_t gq) { GenotypeCall c; c.allele_1 = a; c.allele_2 = b; c.quality = gq; return c; }
static std::string field_of(const std::string& line) { return line.substr(line.rfind('\t') + 1); }
static std::string what_of(const std::function<void()>& f) {
    try { f(); } catch (const std::exception& e) { return e.what(); }
    return "";
}

static void cpu_tests() {
    run("Graph::genotypes_records(RecordFields): the text of hand-made fields, the refusals", [] {
        Variant snp = Variant::from_parts("chr2", 99, "AAAA", "CCCC", {{"C", "G"}}, {}, {{0}, {1}}, {0, 1, 1, 0}, true);
        Variant lone = Variant::from_parts("chr2", 199, "AAAA", "CCCC", {{"C", "CNN"}}, {}, {{0}, {1}}, {0, 1, 1, 0}, true);   // ALT undefined: one defined allele
        Graph graph = Graph::from_parts("chr2", 4, false, {snp}, {{"id-G"}});
        GenotypingResult g;
        g.add_to_likelihood(0, 0, 0.5L); g.add_to_likelihood(0, 1, 0.25L); g.add_to_likelihood(1, 1, 0.0L);
        g.set_coverage(7); g.set_unique_kmers(14);
        // the very likelihoods, normalised: 2/3, 1/3, 0
        GenotypingResult n = g;
        n.normalize();
        const std::vector<std::string> want = graph.genotypes_records({n});
        RecordFields f;
        f.calls = {call(0, 0, 4)};
        f.gl = {gl(-1761, -1), gl(-4771, -1), gl(0, PG_GL_NEG_INF)};
        f.gl_off = {0, 3};
        const std::vector<std::string> got = graph.genotypes_records(f, {7}, {14});
        CHECK(got.size() == 1 && want.size() == 1 && got[0] == want[0]);
        if (got.size() == 1 && want.size() == 1 && got[0] != want[0]) std::printf("    %s\n    %s\n", got[0].c_str(), want[0].c_str());
        CHECK(got.size() == 1 && field_of(got[0]) == "0/0:4:-0.1761,-0.4771,-inf:7");
        // ignore_imputed drops the genotype of a bubble without unique k-mers, not its likelihoods
        CHECK(field_of(graph.genotypes_records(f, {7}, {0}, true)[0]) == ".:.:-0.1761,-0.4771,-inf:7");
        CHECK(graph.genotypes_records(f, {7}, {14}, true)[0] == got[0]);
        f.calls[0] = GenotypeCall();
        CHECK(field_of(graph.genotypes_records(f, {7}, {14})[0]) == ".:.:-0.1761,-0.4771,-inf:7");
        // refusals
        f.gl[1] = gl(0, PG_GL_DEFERRED);
        CHECK(what_of([&] { graph.genotypes_records(f, {7}, {14}); }).find("deferred") != std::string::npos);
        f.gl_off = {0, 2};
        CHECK(what_of([&] { graph.genotypes_records(f, {7}, {14}); }).find("do not fit") != std::string::npos);
        CHECK(what_of([&] { graph.genotypes_records(f, {7, 7}, {14, 14}); }).find("number of variants") != std::string::npos);
        // a record with fewer than two defined alleles: the error of the existing overload
        Graph lonely = Graph::from_parts("chr2", 4, false, {lone}, {{}});
        RecordFields one;
        one.calls = {call(0, 0, 10000)};
        one.gl = {gl(0, 0)};
        one.gl_off = {0, 1};
        GenotypingResult certain;
        certain.add_to_likelihood(0, 0, 1.0L);
        const std::string theirs = what_of([&] { lonely.genotypes_records({certain}); }), ours = what_of([&] { lonely.genotypes_records(one, {7}, {14}); });
        CHECK(theirs.find("too few likelihoods (1)") != std::string::npos && ours == theirs);
        if (ours != theirs) std::printf("    \"%s\" / \"%s\"\n", ours.c_str(), theirs.c_str());
    });
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") {
        cpu_tests();
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (argc < 5 || std::string(argv[1]) != "gpu") { std::printf("usage: test_record_gl_host gpu <index prefix> <reads 1> <reads 2> | cpu\n"); return 2; }
    const std::string prefix = argv[2];
    const std::vector<std::string> both = {argv[3], argv[4]};
    const std::vector<size_t> coverage = {20, 17};

    run("Graph::genotypes_records(genotype_cohort_record_fields) = Graph::genotypes_records(genotype_cohort + normalize), two samples", [&] {
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
            for (size_t v = 0; v < g.size(); ++v) merged += g.get_variant(v).nr_of_records() >= 2;
            for (size_t r = 0; r < plan.nr_of_records(); ++r) {
                bool undefined = false;
                for (uint32_t i = plan.vcf_off[r]; i < plan.vcf_off[r + 1]; ++i) undefined = undefined || plan.vcf_index[i] == 0xFFFF;
                with_undefined += undefined;
            }
            records += plan.nr_of_records();
        }
        CHECK(merged >= 1);           // the input holds what this test is about
        CHECK(with_undefined >= 1);
        ProbabilityTable probs(1, 160, 80, 0.01L);
        auto want = genotype_cohort(m.unique_kmers, counts, &probs, 1.26, false, 0.00001L, 0);
        for (auto& sample : want)
            for (auto& kv : sample)
                for (GenotypingResult& r : kv.second) r.normalize();
        size_t compared = 0, values = 0, finite = 0, no_call = 0, differ = 0;
        for (const bool ignore_imputed : {false, true}) {
            const auto got = genotype_cohort_record_fields(m.unique_kmers, graphs, counts, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
            CHECK(got.size() == 2 && want.size() == 2);
            for (size_t s = 0; s < want.size() && s < got.size(); ++s) {
                CHECK(got[s].size() == want[s].size());
                for (auto& kv : want[s]) {
                    const Graph& graph = graphs.at(kv.first);
                    const std::vector<std::string> lines = graph.genotypes_records(kv.second, ignore_imputed);
                    const auto found = got[s].find(kv.first);
                    CHECK(found != got[s].end());
                    if (found == got[s].end()) continue;
                    std::vector<unsigned short> cov, uk;
                    for (const GenotypingResult& r : kv.second) { cov.push_back(r.coverage()); uk.push_back(r.nr_unique_kmers()); }
                    const RecordFields& f = found->second;
                    const std::vector<std::string> ours = graph.genotypes_records(f, cov, uk, ignore_imputed);
                    CHECK(ours.size() == lines.size() && f.calls.size() == lines.size() && f.gl_off.size() == lines.size() + 1);
                    for (size_t r = 0; r < lines.size() && r < ours.size(); ++r) {
                        CHECK(ours[r] == lines[r]);
                        if (ours[r] != lines[r] && g_failed <= 20) std::printf("    sample %zu record %zu:\n      %s\n      %s\n", s, r, ours[r].c_str(), lines[r].c_str());
                        compared += 1;
                        no_call += lines[r].find("\t.:.:") != std::string::npos;
                        if (s == 1 && !ignore_imputed) {
                            const RecordFields& o = got[0].at(kv.first);
                            for (uint64_t i = f.gl_off[r]; i < f.gl_off[r + 1]; ++i) differ += o.gl[i].mant != f.gl[i].mant || o.gl[i].exp10 != f.gl[i].exp10;
                        }
                    }
                    for (const pg_gl& x : f.gl) { values += 1; finite += x.mant != 0; CHECK(!(x.mant == 0 && x.exp10 == PG_GL_DEFERRED)); }
                    // the file: header and the same lines
                    if (s == 0 && !ignore_imputed) {
                        const std::string path = prefix + "_" + kv.first + "_fields.vcf";
                        graph.write_genotypes(path, f, cov, uk, true, "sample", false);
                        std::FILE* in = std::fopen(path.c_str(), "r");
                        CHECK(in != nullptr);
                        size_t n_lines = 0, n_header = 0;
                        if (in) {
                            char buf[1 << 16];
                            while (std::fgets(buf, sizeof(buf), in)) { n_lines += 1; n_header += buf[0] == '#'; }
                            std::fclose(in);
                        }
                        CHECK(n_lines == ours.size() + n_header && n_header == Graph::genotypes_header("sample").size());
                    }
                }
            }
        }
        CHECK(compared == 4 * records && records > 100 && values > 3 * compared && finite > values / 2 && differ > 0);
        std::printf("  %zu records (%zu merged bubbles, %zu records with an undefined allele), %zu lines compared, %zu GL values, %zu finite, %zu differ between "
                    "the samples, %zu lines without a call\n", records, merged, with_undefined, compared, values, finite, differ, no_call);
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
