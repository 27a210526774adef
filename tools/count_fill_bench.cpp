// count_fill_bench.cpp — the C++ side of tools/bench_count_fill.py: one process, one count(), one JSON line per measurement.
//   count_fill_bench <index prefix> <reads> <kmer coverage>
// The host route (table to the host, fill_read_kmercounts_all at 16 threads, SampleCounts::of) against the count plan
// (DeviceCountPlan::fill / fill_job) on the same counter after the same count.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/pangenie_counts.h"
#include "../pangenie_amd/host/cereal_io.hpp"
#include "../pangenie_amd/host/kmer_counts.hpp"

using namespace pangenie;
using Clock = std::chrono::steady_clock;
static double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

int main(int argc, char** argv) {
    if (argc < 4) { std::printf("usage: count_fill_bench <index prefix> <reads> <kmer coverage>\n"); return 2; }
    const std::string prefix = argv[1], reads = argv[2];
    const size_t coverage = (size_t)std::stoul(argv[3]);
    try {
        UniqueKmersMap index = load_unique_kmers_map(prefix + "_UniqueKmersMap.cereal"), host_index = load_unique_kmers_map(prefix + "_UniqueKmersMap.cereal");
        const size_t k = index.kmersize;
        {
            DeviceKmerCounter warm(k, true);   // (the first device call of a process loads the code object)
            warm.add_target(std::string(k, 'A'));
            (void)warm.targets();
        }
        // once per index: the separate registration pass of the host route against the plan's constructor (which registers too)
        {
            DeviceKmerCounter c(k);
            const auto t0 = Clock::now();
            for (const auto& kv : index.unique_kmers) c.add_targets_from_table(prefix + "_" + kv.first + "_kmers.tsv.gz");
            const size_t targets = c.targets();
            std::printf("{\"what\": \"add_targets_from_table_alone\", \"seconds\": %.4f, \"targets\": %zu}\n", since(t0), targets);
        }
        DeviceKmerCounter counter(k);
        auto t0 = Clock::now();
        DeviceCountPlan plan(counter, index, prefix, true);
        const double construct_s = since(t0);
        uint64_t n_k = 0, n_f = 0, unresolved = 0, plan_bytes = 0, cap = 0;
        pg_count_plan_stats(static_cast<pg_count_plan*>(plan.handle()), &n_k, &n_f, &unresolved, &plan_bytes);
        pg_kmer_counter_capacity(static_cast<pg_kmer_counter*>(counter.handle()), &cap);
        size_t n_v = 0;
        for (const auto& kv : index.unique_kmers) n_v += kv.second.size();
        std::printf("{\"what\": \"plan_construction\", \"seconds\": %.4f, \"unique_kmers\": %llu, \"flanking_kmers\": %llu, \"variants\": %zu, \"plan_device_bytes\": %llu, \"table_bytes\": %llu}\n",
                    construct_s, (unsigned long long)n_k, (unsigned long long)n_f, n_v, (unsigned long long)plan_bytes, (unsigned long long)(cap * 16));
        t0 = Clock::now();
        counter.count(reads);
        std::printf("{\"what\": \"count\", \"seconds\": %.4f, \"windows\": %zu}\n", since(t0), counter.kmers_seen());
        std::fflush(stdout);
        // the count plan first (nothing of the table is on the host yet), three fills
        SampleCounts got;
        for (int round = 0; round < 3; ++round) {
            t0 = Clock::now();
            got = plan.fill(coverage);
            std::printf("{\"what\": \"plan_fill\", \"round\": %d, \"seconds\": %.5f, \"kernel_ms\": %.4f, \"pcie_bytes\": %llu}\n", round, since(t0), plan.last_fill_ms(),
                        (unsigned long long)(2 * (n_k + n_v)));
        }
        // fill_job: a cohort job of one sample over the index
        {
            std::vector<FlatContig> flat(index.unique_kmers.size());
            std::vector<pg_contig_batch> batches;
            std::vector<const uint16_t*> kc, cv;
            size_t c = 0;
            for (auto& kv : index.unique_kmers) {
                flatten(&kv.second, nullptr, flat[c]);
                batches.push_back(flat[c].batch);
                kc.push_back(flat[c].batch.kmer_count);
                cv.push_back(flat[c].batch.coverage);
                c += 1;
            }
            pg_sample_counts row{kc.data(), cv.data()};
            ProbabilityTable probs(coverage / 4, coverage * 4, coverage * 2, 0.01L);
            pg_hmm_params prm{};
            prm.effective_N = 0.00001L; prm.recombrate = 1.26; prm.run_genotyping = 1;
            char err[512] = {0};
            pg_job* job = nullptr;
            if (pg_cohort_new(0, (uint32_t)batches.size(), batches.data(), 1, &row, probs.handle(), &prm, &job, err, sizeof err) != PG_OK) { std::fprintf(stderr, "pg_cohort_new: %s\n", err); return 1; }
            for (int round = 0; round < 3; ++round) {
                t0 = Clock::now();
                plan.fill_job(job, 0, coverage);
                std::printf("{\"what\": \"plan_fill_job\", \"round\": %d, \"seconds\": %.5f, \"kernel_ms\": %.4f, \"pcie_bytes\": %llu}\n", round, since(t0), plan.last_fill_ms(),
                            (unsigned long long)(2 * n_v));
            }
            pg_job_destroy(job);
        }
        std::fflush(stdout);
        // the host route on the same counter: table fetch (first getKmerAbundance), the loop at 16 threads, SampleCounts::of
        t0 = Clock::now();
        try { (void)counter.getKmerAbundance(std::string(k, 'A')); } catch (const std::runtime_error&) {}   // (strict: the fetch comes first)
        const double fetch_s = since(t0);
        t0 = Clock::now();
        fill_read_kmercounts_all(&host_index, counter, prefix, coverage, 16);
        const double loop_s = since(t0);
        t0 = Clock::now();
        const SampleCounts want = SampleCounts::of(host_index.unique_kmers);
        const double of_s = since(t0);
        const bool same = got.kmer_count == want.kmer_count && got.coverage == want.coverage;
        std::printf("{\"what\": \"host_route\", \"seconds\": %.4f, \"table_fetch_s\": %.4f, \"fill_read_kmercounts_all_16_threads_s\": %.4f, \"sample_counts_of_s\": %.4f, \"pcie_bytes\": %llu, \"plan_fill_equal\": %s}\n",
                    fetch_s + loop_s + of_s, fetch_s, loop_s, of_s, (unsigned long long)(cap * 16), same ? "true" : "false");
        return same ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "count_fill_bench: %s\n", e.what());
        return 1;
    }
}
