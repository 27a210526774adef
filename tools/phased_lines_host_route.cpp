// phased_lines_host_route.cpp — the phasing VCF of a cohort ON THE HOST, in C++ on T threads: what a caller does behind
// pg_job_fetch_all where the device forms neither the GT:KC column nor the lines (route (a) of tools/bench_phased_lines.py,
// which builds this as a shared library over libpangenie_host and calls it).  Per chain one GenotypingResult per bubble from the
// fetched haplotypes, kept flags, k-mer counts and coverage, Graph::phasing_records on them — Variant::records,
// get_specific_likelihoods and an ostringstream per record —, the last column of every line; then the join of the samples'
// columns behind Graph::phasing_fixed_columns, as tools/record_lines_host_join.cpp joins (lengths, their sum, copies).
//
// The graphs are made here from the benchmark's synthetic panel: every bubble one record of n_alleles alleles (REF "A", ALT a
// "C" and a times "A", or "N..." where `undefined` says so), the bubble allele of every panel path.  Their record plan is the
// identity plan the benchmark gives the device.
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../pangenie_amd/host/graph_io.hpp"

using namespace pangenie;

namespace {

struct Graphs {
    std::vector<Graph> graph;
    std::vector<std::vector<std::string>> fixed;   // (pl_fixed_columns)
};

template <class F>
void on_threads(int T, uint64_t n, F f) {
    if (T <= 1) { f(0, n); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back([=] { f(n * t / T, n * (t + 1) / T); });
    for (std::thread& t : pool) t.join();
}

}  // namespace

extern "C" void* pl_graphs_new(uint32_t n_contigs, const uint32_t* V, uint32_t H, const uint32_t* const* allele_off, const uint8_t* const* undefined,
                               const uint16_t* const* path_allele) {
    Graphs* g = new Graphs;
    try {
        for (uint32_t k = 0; k < n_contigs; ++k) {
            std::vector<Variant> variants;
            for (uint32_t v = 0; v < V[k]; ++v) {
                const uint32_t a0 = allele_off[k][v], nA = allele_off[k][v + 1] - a0;
                std::vector<std::string> alleles;
                std::vector<std::vector<unsigned short>> combinations;
                for (uint32_t a = 0; a < nA; ++a) {
                    alleles.push_back(a == 0 ? "A" : (undefined[k][a0 + a] ? "N" : "C") + std::string(a, 'A'));
                    combinations.push_back({(unsigned short)a});
                }
                std::vector<unsigned short> paths(path_allele[k] + (size_t)v * H, path_allele[k] + (size_t)(v + 1) * H);
                variants.push_back(Variant::from_parts("chr" + std::to_string(k + 1), 1000 * (size_t)v + 100, "", "", {alleles}, {}, combinations, paths, false));
            }
            g->graph.push_back(Graph::from_parts("chr" + std::to_string(k + 1), 31, false, variants, std::vector<std::vector<std::string>>(V[k])));
        }
    } catch (const std::exception&) { delete g; return nullptr; }
    g->fixed.resize(n_contigs);
    return g;
}
extern "C" void pl_graphs_free(void* h) { delete (Graphs*)h; }

// CHROM .. INFO, GT:KC of contig k under `uk` [V]: the bytes in all (call with bytes == null first), off [R + 1]; kept for pl_host_route
extern "C" uint64_t pl_fixed_columns(void* h, uint32_t k, const uint16_t* uk, uint64_t* off, char* bytes) {
    Graphs* g = (Graphs*)h;
    const Graph& graph = g->graph[k];
    g->fixed[k] = graph.phasing_fixed_columns(std::vector<unsigned short>(uk, uk + graph.size()));
    uint64_t at = 0;
    for (size_t r = 0; r < g->fixed[k].size(); ++r) {
        if (off) off[r] = at;
        if (bytes) memcpy(bytes + at, g->fixed[k][r].data(), g->fixed[k][r].size());
        at += g->fixed[k][r].size();
    }
    if (off) off[g->fixed[k].size()] = at;
    return at;
}

// Chains are sample-major (chain = sample * n_contigs + contig); hap1 / hap2 / kept / n_kmers / coverage [S * n_contigs] arrays of
// [V] each, as pg_job_fetch_all filled them.  seconds[0] = the columns (Graph::phasing_records per chain), seconds[1] = the
// join.  Returns the bytes written; out_off [n_lines + 1].
extern "C" uint64_t pl_host_route(void* h, uint32_t n_contigs, uint32_t S, const uint16_t* const* hap1, const uint16_t* const* hap2, const uint8_t* const* kept,
                                  const uint16_t* const* n_kmers, const uint16_t* const* coverage, int ignore_imputed, int threads, uint64_t* out_off, char* out,
                                  double* seconds) {
    Graphs* g = (Graphs*)h;
    const size_t n_chains = (size_t)S * n_contigs;
    std::vector<std::vector<std::string>> column(n_chains);
    const auto t0 = std::chrono::steady_clock::now();
    {
        std::atomic<size_t> next(0);
        std::vector<std::thread> pool;
        auto work = [&] {
            for (size_t c; (c = next.fetch_add(1)) < n_chains;) {
                const Graph& graph = g->graph[c % n_contigs];
                std::vector<GenotypingResult> results(graph.size());
                for (size_t v = 0; v < results.size(); ++v) {
                    if (kept[c][v]) { results[v].add_first_haplotype_allele(hap1[c][v]); results[v].add_second_haplotype_allele(hap2[c][v]); }
                    results[v].set_unique_kmers(n_kmers[c][v]);
                    results[v].set_coverage(coverage[c][v]);
                }
                for (const std::string& line : graph.phasing_records(results, ignore_imputed != 0)) column[c].push_back(line.substr(line.rfind('\t') + 1));
            }
        };
        if (threads <= 1) work();
        else {
            for (int t = 0; t < threads; ++t) pool.emplace_back(work);
            for (std::thread& t : pool) t.join();
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<uint64_t> line_first(n_contigs + 1, 0);
    for (uint32_t k = 0; k < n_contigs; ++k) line_first[k + 1] = line_first[k] + g->fixed[k].size();
    const uint64_t n = line_first.back();
    auto for_lines = [&](uint64_t l0, uint64_t l1, auto f) {
        uint32_t k = 0;
        for (uint64_t l = l0; l < l1; ++l) {
            while (l >= line_first[k + 1]) ++k;
            f(k, l - line_first[k], l);
        }
    };
    on_threads(threads, n, [&](uint64_t l0, uint64_t l1) {
        for_lines(l0, l1, [&](uint32_t k, uint64_t r, uint64_t l) {
            uint64_t len = g->fixed[k][r].size() + 1;
            for (uint32_t s = 0; s < S; ++s) len += column[(size_t)s * n_contigs + k][r].size() + 1;
            out_off[l + 1] = len;
        });
    });
    out_off[0] = 0;
    for (uint64_t l = 0; l < n; ++l) out_off[l + 1] += out_off[l];
    on_threads(threads, n, [&](uint64_t l0, uint64_t l1) {
        for_lines(l0, l1, [&](uint32_t k, uint64_t r, uint64_t l) {
            char* p = out + out_off[l];
            memcpy(p, g->fixed[k][r].data(), g->fixed[k][r].size());
            p += g->fixed[k][r].size();
            for (uint32_t s = 0; s < S; ++s) {
                const std::string& t = column[(size_t)s * n_contigs + k][r];
                *p++ = '\t';
                memcpy(p, t.data(), t.size());
                p += t.size();
            }
            *p = '\n';
        });
    });
    const auto t2 = std::chrono::steady_clock::now();
    if (seconds) { seconds[0] = std::chrono::duration<double>(t1 - t0).count(); seconds[1] = std::chrono::duration<double>(t2 - t1).count(); }
    return out_off[n];
}
