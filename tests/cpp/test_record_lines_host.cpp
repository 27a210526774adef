// test_record_lines_host.cpp — whole multi-sample VCF lines joined on the device (pangenie_amd/host/graph_io.hpp: RecordLines,
// Graph::genotypes_fixed_columns, compose_record_lines, genotype_cohort_record_lines, Graph::write_genotypes(RecordLines);
// DESIGN.md 4e-7) against the single-sample lines of Graph::genotypes_records(RecordText).  Text for text, column for column.
//   test_record_lines_host cpu <Graph archive>
//       the fixed columns are what every line of genotypes_records begins with; the multi-sample header; the host's
//       composition of a line the device left out; write_genotypes(RecordLines) on hand-made bytes; no device
//   test_record_lines_host counted <UniqueKmersMap archive with read counts> <Graph archive> <cov min> <cov max> <count max>
//       the counts the archive holds as one sample, and the same counts as two samples
//   test_record_lines_host gpu <index prefix> <reads of sample 1> <reads of sample 2>
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

// a hand-made text of R records: sample s, record r (never empty)
static RecordText made_text(size_t R, size_t s, const std::vector<unsigned short>& uk) {
    RecordText t;
    t.off.assign(1, 0);
    for (size_t r = 0; r < R; ++r) {
        t.bytes += std::to_string(s) + "/" + std::to_string(r % 3) + ":" + std::to_string(r) + ":-0.1,-0.2,-inf:" + std::to_string((r * 7 + s) % 60);
        t.off.push_back(t.bytes.size());
    }
    t.unique_kmers = uk;
    return t;
}

static void cpu_tests(const std::string& graph_archive) {
    const Graph graph = Graph::load(graph_archive);
    const size_t R = graph.record_plan().nr_of_records();
    std::vector<unsigned short> uk(graph.size());
    for (size_t v = 0; v < uk.size(); ++v) uk[v] = (unsigned short)((v * 13) % 301);
    run("Graph::genotypes_fixed_columns: what every line of genotypes_records(RecordText) begins with", [&] {
        const std::vector<std::string> fixed = graph.genotypes_fixed_columns(uk);
        const RecordText t = made_text(R, 0, uk);
        const std::vector<std::string> lines = graph.genotypes_records(t);
        CHECK(R >= 2 && fixed.size() == R && lines.size() == R);
        size_t ok = 0;
        for (size_t r = 0; r < R && r < fixed.size() && r < lines.size(); ++r) {
            const std::string want = fixed[r] + '\t' + t.bytes.substr(t.off[r], t.off[r + 1] - t.off[r]);
            ok += lines[r] == want;
            if (lines[r] != want && ok + 5 > r) std::printf("    record %zu:\n      %s\n      %s\n", r, lines[r].c_str(), want.c_str());
            const std::vector<std::string> cols = split(fixed[r], '\t');
            CHECK(cols.size() == 9 && cols[8] == "GT:GQ:GL:KC" && cols[7].find(";UK=") != std::string::npos);
        }
        CHECK(ok == R);
        CHECK(what_of([&] { graph.genotypes_fixed_columns(std::vector<unsigned short>(uk.size() + 1, 0)); }).find("number of variants") != std::string::npos);
    });
    run("Graph::genotypes_header(samples): the names joined by tabs", [&] {
        const std::vector<std::string> one = Graph::genotypes_header("a", "20240101"), three = Graph::genotypes_header(std::vector<std::string>{"a", "b", "c"}, "20240101");
        CHECK(one.size() == three.size() && three.back() == one.back() + "\tb\tc");
        for (size_t i = 0; i + 1 < one.size() && i + 1 < three.size(); ++i) CHECK(one[i] == three[i]);
        CHECK(Graph::genotypes_header(std::vector<std::string>{"a"}, "20240101") == one);
    });
    run("compose_record_lines: a line the device left out is put together here, every other line is copied", [&] {
        // 50 hand-made records (the region fixture's graph has two): prefixes of any bytes, one of them empty
        const size_t R = 50;
        std::vector<std::string> fixed;
        for (size_t r = 0; r < R; ++r) fixed.push_back(r == 10 ? "" : "chrZ\t" + std::to_string(100 * r + 1) + "\t.\tA\tC\t.\tPASS\tAF=0.5;UK=" + std::to_string(r) + "\tGT:GQ:GL:KC");
        const RecordText t0 = made_text(R, 0, {}), t1 = made_text(R, 1, {});
        std::vector<std::string> singles[2];
        for (size_t r = 0; r < R; ++r) {
            singles[0].push_back(fixed[r] + '\t' + t0.bytes.substr(t0.off[r], t0.off[r + 1] - t0.off[r]));
            singles[1].push_back(fixed[r] + '\t' + t1.bytes.substr(t1.off[r], t1.off[r + 1] - t1.off[r]));
        }
        // the device's lines: every seventh left out, the others marked so that a copy can be told from a composition
        RecordLines device;
        device.off.assign(1, 0);
        for (size_t r = 0; r < R; ++r) {
            if (r % 7 != 3) device.bytes += "device line " + std::to_string(r) + "\n";
            device.off.push_back(device.bytes.size());
        }
        const RecordLines got = compose_record_lines(fixed, {&t0, &t1}, device);
        CHECK(got.off.size() == R + 1 && got.off[0] == 0 && got.off.back() == got.bytes.size());
        size_t composed = 0;
        for (size_t r = 0; r < R && r + 1 < got.off.size(); ++r) {
            const std::string line = got.bytes.substr(got.off[r], got.off[r + 1] - got.off[r]);
            if (r % 7 != 3) { CHECK(line == "device line " + std::to_string(r) + "\n"); continue; }
            composed += 1;
            CHECK(line == singles[0][r] + '\t' + split(singles[1][r], '\t').back() + '\n');
        }
        CHECK(composed >= R / 7);
        // ... and on the graph's own records: composed from its fixed columns, a line is genotypes_records' line with a column more
        const std::vector<std::string> gfixed = graph.genotypes_fixed_columns(uk);
        const size_t GR = gfixed.size();
        const RecordText g0 = made_text(GR, 0, uk), g1 = made_text(GR, 1, uk);
        RecordLines gnone;
        gnone.off.assign(GR + 1, 0);
        const RecordLines glines = compose_record_lines(gfixed, {&g0, &g1}, gnone);
        const std::vector<std::string> ga = graph.genotypes_records(g0), gb = graph.genotypes_records(g1);
        for (size_t r = 0; r < GR && r + 1 < glines.off.size(); ++r)
            CHECK(glines.bytes.substr(glines.off[r], glines.off[r + 1] - glines.off[r]) == ga[r] + '\t' + split(gb[r], '\t').at(9) + '\n');
        // nothing left out: the device's bytes as they are
        RecordLines all;
        all.off.assign(1, 0);
        for (size_t r = 0; r < R; ++r) { all.bytes += "x\n"; all.off.push_back(all.bytes.size()); }
        const RecordLines same = compose_record_lines(fixed, {&t0}, all);
        CHECK(same.bytes == all.bytes && same.off == all.off);
        // a sample whose text of such a record is empty too: fewer than three values, as everywhere
        RecordText hole = t1;
        hole.off[4] = hole.off[3];   // (record 3, one of those left out, is empty: its bytes go to record 4)
        CHECK(what_of([&] { compose_record_lines(fixed, {&t0, &hole}, device); }).find("too few likelihoods") != std::string::npos);
        RecordLines wrong = device;
        wrong.off.pop_back();
        CHECK(what_of([&] { compose_record_lines(fixed, {&t0}, wrong); }).find("do not fit") != std::string::npos);
        RecordText brief = t0;
        brief.off.pop_back();
        CHECK(what_of([&] { compose_record_lines(fixed, {&brief}, device); }).find("does not fit") != std::string::npos);
    });
    run("Graph::write_genotypes(RecordLines): header and body, appended without a header, the refusals", [&] {
        const std::vector<std::string> fixed = graph.genotypes_fixed_columns(uk);
        const RecordText t0 = made_text(R, 0, uk), t1 = made_text(R, 1, uk);
        RecordLines none;
        none.off.assign(R + 1, 0);
        const RecordLines lines = compose_record_lines(fixed, {&t0, &t1}, none);   // (every line the host's)
        const std::string path = "test_record_lines_host.tmp.vcf";
        graph.write_genotypes(path, lines, true, {"s0", "s1"});
        std::vector<std::string> got = lines_of_file(path);
        const size_t H = Graph::genotypes_header("x").size();
        CHECK(got.size() == H + R && got[H - 1] == Graph::genotypes_header(std::vector<std::string>{"s0", "s1"}).back());
        const std::vector<std::string> a = graph.genotypes_records(t0), b = graph.genotypes_records(t1);
        size_t ok = 0;
        for (size_t r = 0; r < R && H + r < got.size(); ++r) ok += got[H + r] == a[r] + '\t' + split(b[r], '\t').at(9);
        CHECK(ok == R);
        graph.write_genotypes(path, lines, false, {"s0", "s1"});
        got = lines_of_file(path);
        CHECK(got.size() == H + 2 * R && got[H + R] == got[H]);
        std::remove(path.c_str());
        RecordLines bad = lines;
        bad.off[1] = bad.off[0];
        CHECK(what_of([&] { graph.write_genotypes(path, bad, true, {"s0", "s1"}); }).find("empty or unfinished") != std::string::npos);
        bad = lines;
        bad.off.pop_back();
        CHECK(what_of([&] { graph.write_genotypes(path, bad, true, {"s0", "s1"}); }).find("do not fit") != std::string::npos);
        CHECK(lines_of_file(path).empty());   // (refused before the file is touched)
    });
    run("genotype_cohort_record_lines refuses a missing graph before any job, and does nothing without chromosomes", [] {
        std::vector<unsigned short> alleles = {0, 1};
        std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>> chromosomes, empty;
        chromosomes["chr2"] = {std::make_shared<BiallelicUniqueKmers>(99, alleles)};
        std::map<std::string, Graph> none;
        std::vector<SampleCounts> samples(1);
        ProbabilityTable probs(1, 160, 80, 0.01L);
        CHECK(what_of([&] { genotype_cohort_record_lines(chromosomes, none, samples, &probs); }).find("no graph of chr2") != std::string::npos);
        CHECK(genotype_cohort_record_lines(empty, none, samples, &probs).empty());
    });
}

// every line of the device route, split at tabs, against the single-sample lines of genotypes_records(text_s); then the file
static void lines_against_singles(const std::function<UniqueKmersMap()>& fresh, const std::map<std::string, Graph>& graphs, const std::vector<SampleCounts>& counts,
                                  ProbabilityTable& probs, size_t records) {
    const size_t S = counts.size();
    const std::string name = "genotype_cohort_record_lines, " + std::to_string(S) + " sample(s): columns 1-9 and column 9 + s of genotypes_records(genotype_cohort_record_text)";
    run(name.c_str(), [&] {
        size_t compared = 0, bytes = 0, no_call = 0;
        for (const bool ignore_imputed : {false, true}) {
            UniqueKmersMap m = fresh(), other = fresh();
            const auto text = genotype_cohort_record_text(other.unique_kmers, graphs, counts, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
            const auto lines = genotype_cohort_record_lines(m.unique_kmers, graphs, counts, &probs, 1.26, false, 0.00001L, 0, ignore_imputed);
            CHECK(text.size() == S && lines.size() == graphs.size());
            for (const auto& kv : lines) {
                const Graph& graph = graphs.at(kv.first);
                const RecordLines& l = kv.second;
                std::vector<std::vector<std::string>> singles(S);
                for (size_t s = 0; s < S; ++s) singles[s] = graph.genotypes_records(text[s].at(kv.first));
                const size_t R = singles[0].size();
                CHECK(l.off.size() == R + 1 && l.off[0] == 0 && l.off.back() == l.bytes.size());
                if (l.off.size() != R + 1) continue;
                for (size_t r = 0; r < R; ++r) {
                    CHECK(l.off[r + 1] > l.off[r] && l.bytes[l.off[r + 1] - 1] == '\n');
                    if (l.off[r + 1] <= l.off[r]) continue;
                    const std::vector<std::string> cols = split(l.bytes.substr(l.off[r], l.off[r + 1] - l.off[r] - 1), '\t');
                    CHECK(cols.size() == 9 + S);
                    if (cols.size() != 9 + S) continue;
                    bool same = true;
                    for (size_t s = 0; s < S; ++s) {
                        const std::vector<std::string> one = split(singles[s][r], '\t');
                        same = same && one.size() == 10 && one[9] == cols[9 + s];
                        for (size_t k = 0; k < 9 && same; ++k) same = one[k] == cols[k];
                        no_call += cols[9 + s].rfind(".:.:", 0) == 0;
                    }
                    CHECK(same);
                    if (!same && g_failed <= 20) std::printf("    %s record %zu:\n      %s      %s\n", kv.first.c_str(), r, l.bytes.substr(l.off[r], l.off[r + 1] - l.off[r]).c_str(), singles[0][r].c_str());
                    compared += 1;
                }
                bytes += l.bytes.size();
                // the file: read back against lines put together from the single-sample files
                if (ignore_imputed) continue;
                const std::string path = "test_record_lines_host." + kv.first + ".tmp.vcf";
                std::vector<std::string> names;
                std::vector<std::vector<std::string>> files(S);
                for (size_t s = 0; s < S; ++s) {
                    names.push_back("sample" + std::to_string(s));
                    graph.write_genotypes(path, text[s].at(kv.first), true, names.back());
                    files[s] = lines_of_file(path);
                }
                graph.write_genotypes(path, l, true, names);
                const std::vector<std::string> got = lines_of_file(path);
                std::remove(path.c_str());
                CHECK(got.size() == files[0].size() && got.size() > R);
                size_t ok = 0;
                for (size_t i = 0; i < got.size() && i < files[0].size(); ++i) {
                    std::string want = files[0][i];
                    if (want.rfind("##", 0) != 0)
                        for (size_t s = 1; s < S; ++s) want += '\t' + split(files[s][i], '\t').at(9);
                    ok += got[i] == want;
                }
                CHECK(ok == got.size());
            }
        }
        CHECK(compared == 2 * records && bytes > 20 * compared * S);
        std::printf("  %zu lines of %zu sample(s) compared, %zu bytes, %zu columns without a call\n", compared, S, bytes, no_call);
    });
}

int main(int argc, char** argv) {
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (mode == "cpu" && argc >= 3) {
        cpu_tests(argv[2]);
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (mode == "counted" && argc >= 7) {
        const std::string archive = argv[2], graph_archive = argv[3];
        ProbabilityTable probs((unsigned)std::atoi(argv[4]), (unsigned)std::atoi(argv[5]), (unsigned)std::atoi(argv[6]), 0.01L);
        auto fresh = [&] { return load_unique_kmers_map(archive); };
        const UniqueKmersMap index = fresh();
        std::map<std::string, Graph> graphs;
        size_t records = 0;
        for (const auto& kv : index.unique_kmers) {
            graphs[kv.first] = Graph::load(graph_archive);
            records += graphs[kv.first].record_plan().nr_of_records();
        }
        const SampleCounts one = SampleCounts::of(index.unique_kmers);
        lines_against_singles(fresh, graphs, {one}, probs, records);
        lines_against_singles(fresh, graphs, {one, one}, probs, records);
        std::printf("%d checks, %d failed\n", g_checks, g_failed);
        return g_failed ? 1 : 0;
    }
    if (mode != "gpu" || argc < 5) {
        std::printf("usage: test_record_lines_host cpu <graph> | counted <archive> <graph> <cov min> <cov max> <count max> | gpu <index prefix> <reads 1> <reads 2>\n");
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
    lines_against_singles(fresh, graphs, counts, probs, records);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
