// kmer_counter_bench.cpp — the C++ side of tools/bench_kmer_counter.py: one process, one JSON line per measurement.
//   kmer_counter_bench <k> <path_segments.fasta> <reads> <kmers.tsv.gz> [<kmers.tsv.gz> ...]
// Rates are bytes of the read FILE per second of wall time (the same numerator for every line), windows per second for the
// kernel alone.
#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/pangenie_kmers.h"
#include "../pangenie_amd/host/kmer_counts.hpp"

using namespace pangenie;
using Clock = std::chrono::steady_clock;
static double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

int main(int argc, char** argv) {
    if (argc < 5) { std::printf("usage: kmer_counter_bench <k> <path_segments.fasta> <reads> <kmers.tsv.gz> [...]\n"); return 2; }
    const size_t k = (size_t)std::stoul(argv[1]);
    const std::string segments = argv[2], reads = argv[3];
    std::vector<std::string> tables(argv + 4, argv + argc);
    struct stat st;
    if (stat(reads.c_str(), &st) != 0) { std::fprintf(stderr, "cannot stat %s\n", reads.c_str()); return 1; }
    const double file_bytes = (double)st.st_size;
    try {
        // 1. the reader alone, twice (the first pass also warms the page cache for everyone after it)
        std::string all_text;   // the batches of the second pass, kept for the kernel-alone runs
        for (int pass = 0; pass < 2; ++pass) {
            const auto t0 = Clock::now();
            size_t batches = 0;
            const size_t bytes = for_each_read_batch(reads, [&](std::string_view) { batches += 1; });
            const double s = since(t0);
            std::printf("{\"what\": \"reader_alone\", \"pass\": %d, \"seconds\": %.4f, \"file_bytes\": %.0f, \"batch_bytes\": %zu, \"batches\": %zu, \"bytes_per_s\": %.4g}\n",
                        pass, s, file_bytes, bytes, batches, file_bytes / s);
            std::fflush(stdout);
        }
        for_each_read_batch(reads, [&](std::string_view b) { all_text.append(b); });
        // 2. TargetedKmerCounter::count at 1 and at 16 threads: targets = the graph's segments; the first count builds the
        //    table too (that is what the call does), the second one runs on the built table
        std::vector<size_t> host_hist;
        size_t host_seen = 0, host_targets = 0;
        const bool device_only = std::getenv("PG_KMER_BENCH_DEVICE_ONLY") != nullptr;   // (profiled runs: tools/profile.sh kmers)
        for (unsigned threads : {16u, 1u}) {
            if (device_only) break;
            TargetedKmerCounter c(k, true);
            const auto tr = Clock::now();
            c.add_targets_from_sequences(segments);
            const double reg = since(tr);
            const int rounds = threads == 1 ? 1 : 2;
            for (int round = 0; round < rounds; ++round) {
                const auto t0 = Clock::now();
                c.count(reads, threads);
                const double s = since(t0);
                std::printf("{\"what\": \"host_targeted_count\", \"threads\": %u, \"table_built_in_call\": %s, \"seconds\": %.4f, \"register_seconds\": %.4f, \"bytes_per_s\": %.4g, \"targets\": %zu, \"windows\": %zu}\n",
                            threads, round == 0 ? "true" : "false", s, reg, file_bytes / s, c.targets(), c.kmers_seen() / (size_t)(round + 1));
                std::fflush(stdout);
                if (threads == 16 && round == 0) { host_hist = c.abundance_histogram(200); host_seen = c.kmers_seen(); host_targets = c.targets(); }
            }
        }
        // 3. DeviceKmerCounter::count end to end: pageable file to synced counts; first call (table built in it), then the
        //    next samples over the same table (reset_counts)
        {
            DeviceKmerCounter warm(k, true);   // (the first device call of a process loads the code object)
            warm.add_target(std::string(k, 'A'));
            (void)warm.targets();
            DeviceKmerCounter c(k, true);
            const auto tr = Clock::now();
            c.add_targets_from_sequences(segments);
            const double reg = since(tr);
            for (int round = 0; round < 4; ++round) {
                if (round) c.reset_counts();
                const auto t0 = Clock::now();
                c.count(reads, 16);
                const double s = since(t0);
                const bool same = device_only || (c.abundance_histogram(200) == host_hist && c.kmers_seen() == host_seen && c.targets() == host_targets);
                std::printf("{\"what\": \"device_count_end_to_end\", \"round\": %d, \"table_built_in_call\": %s, \"seconds\": %.4f, \"register_seconds\": %.4f, \"bytes_per_s\": %.4g, \"targets\": %zu, \"windows\": %zu, \"same_as_host\": %s}\n",
                            round, round == 0 ? "true" : "false", s, reg, file_bytes / s, c.targets(), c.kmers_seen(), same ? "true" : "false");
                std::fflush(stdout);
            }
            const auto tf = Clock::now();
            (void)c.getKmerAbundance(std::string(k, 'A'));
            std::printf("{\"what\": \"device_table_to_host\", \"seconds\": %.4f}\n", since(tf));
        }
        // 4. the counting kernel alone on text resident in HBM, for both target sets
        for (int set = 0; set < 2; ++set) {
            DeviceKmerCounter c(k, true);
            if (set == 0) c.add_targets_from_sequences(segments);
            else for (const std::string& t : tables) c.add_targets_from_table(t);
            const size_t targets = c.targets();
            double ms[5];
            pg_kmer_counter* h = static_cast<pg_kmer_counter*>(c.handle());
            const int rc = pg_kmer_counter_count_resident(h, all_text.data(), all_text.size(), 5, ms);
            if (rc) { std::fprintf(stderr, "pg_kmer_counter_count_resident: %d %s\n", rc, pg_kmer_last_error()); return 1; }
            const double windows = (double)c.kmers_seen() / 5.0;
            const std::vector<size_t> hist = c.abundance_histogram(1u << 20);
            double hits = 0;
            for (size_t n = 1; n < hist.size(); ++n) hits += (double)n * (double)hist[n];
            double best = ms[1];
            for (int r = 1; r < 5; ++r) best = ms[r] < best ? ms[r] : best;
            std::printf("{\"what\": \"count_kernel_resident\", \"targets_from\": \"%s\", \"targets\": %zu, \"text_bytes\": %zu, \"windows\": %.0f, \"hit_fraction\": %.4f, \"ms\": [%.3f, %.3f, %.3f, %.3f, %.3f], \"windows_per_s\": %.4g, \"text_bytes_per_s\": %.4g}\n",
                        set == 0 ? "graph segments" : "table k-mers", targets, all_text.size(), windows, hits / 5.0 / windows, ms[0], ms[1], ms[2], ms[3], ms[4],
                        windows / (best * 1e-3), (double)all_text.size() / (best * 1e-3));
            std::fflush(stdout);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "kmer_counter_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
