// test_device_counter.cpp — pangenie::DeviceKmerCounter (pangenie_amd/host/kmer_counts.hpp) against the host counters:
// every expected count comes from ExactKmerCounter or TargetedKmerCounter, every comparison is exact.
//   test_device_counter gpu <golden dir> [<scratch dir>]
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

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
static std::vector<unsigned char> read_file(const std::string& path) {
    std::vector<unsigned char> bytes;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return bytes;
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    return bytes;
}
static void gzip_copy(const std::string& from, const std::string& to) {
    const std::vector<unsigned char> raw = read_file(from);
    gzFile out = gzopen(to.c_str(), "wb");
    if (!out) throw std::runtime_error("cannot write " + to);
    gzwrite(out, raw.data(), (unsigned)raw.size());
    gzclose(out);
}
// the k-mers of a `_kmers.tsv.gz` table
static std::vector<std::string> table_kmers(const std::string& table) {
    std::vector<std::string> all;
    gzFile t = gzopen(table.c_str(), "rb");
    if (!t) throw std::runtime_error("cannot open " + table);
    static char buf[1 << 16];
    std::string line;
    while (gzgets(t, buf, sizeof buf)) {
        line += buf;
        if (line.empty() || line.back() != '\n') continue;
        line.pop_back();
        std::string chrom; size_t start = 0; std::vector<std::string> km, fl; bool header = false;
        parse_kmer_line(line, chrom, start, km, fl, header);
        all.insert(all.end(), km.begin(), km.end());
        all.insert(all.end(), fl.begin(), fl.end());
        line.clear();
    }
    gzclose(t);
    return all;
}

int main(int argc, char** argv) {
    if (argc < 3 || std::string(argv[1]) != "gpu") { std::printf("usage: test_device_counter gpu <golden dir> [<scratch dir>]\n"); return 2; }
    const std::string golden = argv[2], tmp = argc > 3 ? argv[3] : "/tmp";

    run("large target set: DeviceKmerCounter = ExactKmerCounter on every k-mer; FASTA over lines, FASTQ, gzip give the same", [&] {
        // 400 k windows of a pseudo-random sequence registered; reads = 6000 pieces of it, either strand, a few wrong letters and
        // an N now and then
        std::string graph;
        uint64_t x = 0xD1B54A32D192ED03ull;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        for (int i = 0; i < 400030; ++i) graph += "ACGT"[rnd() & 3];
        const std::string fa = tmp + "/pg_dev_big_graph.fa", reads = tmp + "/pg_dev_big_reads.fa";
        { std::FILE* f = std::fopen(fa.c_str(), "w"); std::fprintf(f, ">g\n%s\n", graph.c_str()); std::fclose(f); }
        {
            std::FILE* f = std::fopen(reads.c_str(), "w");
            for (int r = 0; r < 6000; ++r) {
                std::string piece = graph.substr(rnd() % (graph.size() - 200), 100 + rnd() % 100);
                if (r % 2) { std::reverse(piece.begin(), piece.end()); for (char& c : piece) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
                if (r % 7 == 0) piece[rnd() % piece.size()] = "ACGT"[rnd() & 3];
                if (r % 31 == 0) piece[rnd() % piece.size()] = 'N';
                std::fprintf(f, ">r%d\n%s\n", r, piece.c_str());
            }
            std::fclose(f);
        }
        ExactKmerCounter exact(reads, 31);
        TargetedKmerCounter host(31);
        DeviceKmerCounter dev(31);
        CHECK(host.add_targets_from_sequences(fa) == 400000);
        CHECK(dev.add_targets_from_sequences(fa) == 400000);
        host.count(reads, 4);
        dev.count(reads, 4);
        CHECK(dev.targets() == host.targets() && dev.targets() > 399000);
        CHECK(dev.kmers_seen() == host.kmers_seen() && dev.kmers_seen() > 0);
        size_t differ = 0, seen = 0;
        for (size_t i = 0; i + 31 <= graph.size(); ++i) {   // every registered k-mer
            const std::string kmer = graph.substr(i, 31);
            const size_t want = exact.getKmerAbundance(kmer);
            differ += dev.getKmerAbundance(kmer) != want;
            seen += want > 0;
        }
        CHECK(differ == 0);
        CHECK(seen > 150000);
        CHECK(dev.abundance_histogram(100) == host.abundance_histogram(100));
        // the same reads as FASTA with the sequence over several lines, as FASTQ whose quality lines begin with '@', '+' and '>'
        // now and then, and both gzipped: the same counts and the same kmers_seen
        const std::string fa_lines = tmp + "/pg_dev_big_reads_lines.fa", fq = tmp + "/pg_dev_big_reads.fq";
        {
            std::FILE* in = std::fopen(reads.c_str(), "r");
            std::FILE* a = std::fopen(fa_lines.c_str(), "w");
            std::FILE* q = std::fopen(fq.c_str(), "w");
            char line[512];
            int r = 0;
            while (std::fgets(line, sizeof line, in)) {
                if (line[0] == '>') continue;
                std::string seq(line);
                while (!seq.empty() && (seq.back() == '\n' || seq.back() == '\r')) seq.pop_back();
                std::fprintf(a, ">read%d some text\n", r);
                for (size_t i = 0; i < seq.size(); i += 37 + r % 5) std::fprintf(a, "%s\n", seq.substr(i, 37 + r % 5).c_str());
                std::string quality(seq.size(), 'I');
                if (r % 3 == 0) quality[0] = '@';
                if (r % 3 == 1) quality[0] = '+';
                if (r % 7 == 2) quality[0] = '>';
                std::fprintf(q, "@read%d/1\n%s\n+%s\n%s\n", r, seq.c_str(), r % 2 ? "read" : "", quality.c_str());
                r += 1;
            }
            std::fclose(in); std::fclose(a); std::fclose(q);
        }
        gzip_copy(fa_lines, fa_lines + ".gz");
        gzip_copy(fq, fq + ".gz");
        gzip_copy(reads, reads + ".gz");
        for (const std::string& path : {fa_lines, fq, fa_lines + ".gz", fq + ".gz", reads + ".gz"}) {
            DeviceKmerCounter other(31);
            other.add_targets_from_sequences(fa);
            other.count(path, 3);
            CHECK(other.kmers_seen() == host.kmers_seen());
            size_t wrong = 0;
            for (size_t i = 0; i + 31 <= graph.size(); ++i) wrong += other.getKmerAbundance(graph.substr(i, 31)) != exact.getKmerAbundance(graph.substr(i, 31));
            CHECK(wrong == 0);
        }
        // the next sample over the same targets: reset_counts, count again = the same numbers; two files add up
        dev.reset_counts();
        CHECK(dev.kmers_seen() == 0 && dev.getKmerAbundance(graph.substr(0, 31)) == 0 && dev.targets() == host.targets());
        dev.count(fq, 1);
        dev.count(reads + ".gz", 1);
        CHECK(dev.kmers_seen() == 2 * host.kmers_seen());
        size_t wrong = 0;
        for (size_t i = 0; i + 31 <= graph.size(); ++i) wrong += dev.getKmerAbundance(graph.substr(i, 31)) != 2 * exact.getKmerAbundance(graph.substr(i, 31));
        CHECK(wrong == 0);
    });

    run("the golden index: targets from the table, fill_read_kmercounts = the reference's counted archive byte for byte", [&] {
        const std::string table = golden + "/index_chr1_kmers.tsv.gz", reads = golden + "/region-reads.fa";   // (FASTQ despite its name)
        const std::string gz = tmp + "/pg_dev_region_reads.fq.gz";
        gzip_copy(reads, gz);
        const std::vector<std::string> all = table_kmers(table);
        CHECK(all.size() > 100);
        const UniqueKmersMap want = load_unique_kmers_map(golden + "/region_UniqueKmersList.cereal");
        const std::vector<unsigned char> want_bytes = read_file(golden + "/region_UniqueKmersList.cereal");
        CHECK(!want_bytes.empty());
        for (const std::string& path : {reads, gz}) {
            UniqueKmersMap m = load_unique_kmers_map(golden + "/index_UniqueKmersMap.cereal");
            ExactKmerCounter exact(reads, m.kmersize);
            DeviceKmerCounter c(m.kmersize);
            CHECK(c.add_targets_from_table(table) == 2);
            c.count(path, 3);
            CHECK(c.targets() > 100 && c.targets() <= all.size() && c.kmers_seen() > 1000);
            size_t same = 0, nonzero = 0;
            for (const std::string& k : all) { const size_t n = c.getKmerAbundance(k); same += n == exact.getKmerAbundance(k); nonzero += n > 0; }
            CHECK(same == all.size() && nonzero > 50);
            fill_read_kmercounts("chr1", &m, c, table, 18);
            m.runtimes = want.runtimes;
            m.sampling_runtimes = want.sampling_runtimes;
            CHECK(serialize_unique_kmers_map(m) == want_bytes);
            // and through the thread pool around it
            UniqueKmersMap m2 = load_unique_kmers_map(golden + "/index_UniqueKmersMap.cereal");
            fill_read_kmercounts_all(&m2, c, golden + "/index", 18, 4);
            m2.runtimes = want.runtimes;
            m2.sampling_runtimes = want.sampling_runtimes;
            CHECK(serialize_unique_kmers_map(m2) == want_bytes);
        }
    });

    run("strict throws for an unregistered k-mer, lenient answers 0; getKmerAbundance from 8 threads at once", [&] {
        const std::string fa = tmp + "/pg_dev_reads_t.fa";
        { FILE* f = std::fopen(fa.c_str(), "w"); std::fputs(">r1\nACGTAC\nGT\n>r2\nACGNACGTA", f); std::fclose(f); }   // (no final newline)
        TargetedKmerCounter host(4);
        DeviceKmerCounter strict(4), lenient(4, true);
        for (const char* k : {"ACGT", "TACG", "ACGN", "GGGG"}) { host.add_target(k); strict.add_target(k); lenient.add_target(k); }
        host.count(fa, 1); strict.count(fa, 1); lenient.count(fa, 1);
        CHECK(strict.targets() == host.targets() && strict.targets() == 3 && strict.kmers_seen() == host.kmers_seen());
        for (const char* k : {"ACGT", "TACG", "CGTA", "GGGG", "CCCC", "ACGN"}) {
            CHECK(strict.getKmerAbundance(k) == host.getKmerAbundance(k));
            CHECK(lenient.getKmerAbundance(k) == host.getKmerAbundance(k));
        }
        CHECK(strict.getKmerAbundance("ACGT") == 3 && strict.getKmerAbundance("GGGG") == 0);
        std::string said;
        try { strict.getKmerAbundance("GTAC"); } catch (const std::runtime_error& e) { said = e.what(); }
        CHECK(said == "DeviceKmerCounter::getKmerAbundance: GTAC was not registered before the reads were counted");
        CHECK(lenient.getKmerAbundance("GTAC") == 0);
        said.clear();
        try { strict.getKmerAbundance("ACG"); } catch (const std::runtime_error& e) { said = e.what(); }
        CHECK(said == "DeviceKmerCounter::getKmerAbundance: k-mer of length 3, counter holds 4-mers");
        said.clear();
        try { strict.add_target("AAAA"); } catch (const std::runtime_error& e) { said = e.what(); }
        CHECK(said == "DeviceKmerCounter: targets must be registered before the reads are counted");
        bool threw = false;
        try { DeviceKmerCounter bad(33); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
        // 8 threads ask a counter whose table has not been fetched yet
        const std::string table = golden + "/index_chr1_kmers.tsv.gz", reads = golden + "/region-reads.fa";
        const std::vector<std::string> all = table_kmers(table);
        TargetedKmerCounter h31(31);
        DeviceKmerCounter d31(31);
        h31.add_targets_from_table(table); d31.add_targets_from_table(table);
        h31.count(reads, 2); d31.count(reads, 2);
        std::vector<size_t> want;
        for (const std::string& k : all) want.push_back(h31.getKmerAbundance(k));
        std::vector<size_t> wrong(8, 0);
        std::vector<std::thread> pool;
        for (int t = 0; t < 8; ++t)
            pool.emplace_back([&, t] {
                for (int round = 0; round < 20; ++round)
                    for (size_t i = (size_t)t; i < all.size(); i += 3) wrong[(size_t)t] += d31.getKmerAbundance(all[i]) != want[i];
            });
        for (std::thread& t : pool) t.join();
        for (int t = 0; t < 8; ++t) CHECK(wrong[(size_t)t] == 0);
    });

    run("index_path_segments.fasta as target source and as reads: every k-mer seen at least once, as on the host", [&] {
        const std::string seg = golden + "/index_path_segments.fasta";
        TargetedKmerCounter host(31, true);
        DeviceKmerCounter dev(31, true);
        const size_t n = host.add_targets_from_sequences(seg);
        CHECK(n > 0 && dev.add_targets_from_sequences(seg) == n);
        host.count(seg, 2);
        dev.count(seg, 2);
        CHECK(dev.targets() == host.targets() && dev.kmers_seen() == host.kmers_seen() && dev.kmers_seen() == n);
        const std::vector<size_t> hh = host.abundance_histogram(1000), dh = dev.abundance_histogram(1000);
        CHECK(hh == dh);
        size_t seen = 0;
        for (size_t c = 1; c < dh.size(); ++c) seen += dh[c];
        CHECK(seen == dev.targets());   // none at 0 (and none above 1000)
        // k-mer by k-mer over the file's own letters
        const std::vector<unsigned char> raw = read_file(seg);
        std::string text(raw.begin(), raw.end());
        size_t at = 0, asked = 0, differ = 0, unseen = 0;
        while (at < text.size()) {
            size_t nl = text.find('\n', at);
            if (nl == std::string::npos) nl = text.size();
            if (text[at] != '>')
                for (size_t i = at; i + 31 <= nl; ++i) {
                    const std::string k = text.substr(i, 31);
                    if (k.find_first_not_of("ACGTacgt") != std::string::npos) continue;   // (no window: the file has a few N)
                    const size_t got = dev.getKmerAbundance(k);
                    differ += got != host.getKmerAbundance(k);
                    unseen += got == 0;
                    asked += 1;
                }
            at = nl + 1;
        }
        CHECK(asked > 0 && differ == 0 && unseen == 0);
    });

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
