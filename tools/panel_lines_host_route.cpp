// panel_lines_host_route.cpp — the sampled-panel VCF of a sampled cohort ON THE HOST, in C++ on T threads: what a caller does
// behind pg_job_fetch_panel where the device forms neither the haplotype columns nor the lines (route (a) of
// tools/bench_panel_lines.py, which builds this as a shared library over libpangenie_host and calls it).  Per chain one
// SampledPanel per bubble from the fetched kmer_off and path_allele, Graph::sampled_panel_records on them — Variant::records
// and an ostringstream per record —, then the lines of all chains packed, chain after chain, a newline behind each.
//
// The graphs are made here from the benchmark's synthetic panel, as tools/phased_lines_host_route.cpp makes them: every bubble
// one record of n_alleles alleles (REF "A", ALT a "C" and a times "A", or "N..." where `undefined` says so), the bubble allele
// of every panel path.  Their record plan is the identity plan the benchmark gives the device.
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
};

}  // namespace

extern "C" void* pp_graphs_new(uint32_t n_contigs, const uint32_t* V, uint32_t H, const uint32_t* const* allele_off, const uint8_t* const* undefined,
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
    return g;
}
extern "C" void pp_graphs_free(void* h) { delete (Graphs*)h; }

// CHROM .. INFO, GT of contig k with the digits of UK left out: the bytes in all (call with bytes == null first), off [R + 1], slot [R]
extern "C" uint64_t pp_fixed_columns_slotted(void* h, uint32_t k, uint64_t* off, char* bytes, uint32_t* slot) {
    Graphs* g = (Graphs*)h;
    std::vector<uint32_t> slots;
    const std::vector<std::string> fixed = g->graph[k].sampled_panel_fixed_columns_slotted(&slots);
    uint64_t at = 0;
    for (size_t r = 0; r < fixed.size(); ++r) {
        if (off) off[r] = at;
        if (slot) slot[r] = slots[r];
        if (bytes) memcpy(bytes + at, fixed[r].data(), fixed[r].size());
        at += fixed[r].size();
    }
    if (off) off[fixed.size()] = at;
    return at;
}

// Chains are sample-major (chain = sample * n_contigs + contig); kmer_off [S * n_contigs] arrays of [V + 1], path_allele of
// [V x P], as pg_job_fetch_panel filled them.  seconds[0] = Graph::sampled_panel_records per chain, seconds[1] = the packing.
// Returns the bytes written; out_off [n_lines + 1].
extern "C" uint64_t pp_host_route(void* h, uint32_t n_contigs, uint32_t S, uint32_t P, const uint32_t* const* kmer_off, const uint16_t* const* path_allele,
                                  int threads, uint64_t* out_off, char* out, double* seconds) {
    Graphs* g = (Graphs*)h;
    const size_t n_chains = (size_t)S * n_contigs;
    std::vector<std::vector<std::string>> lines(n_chains);
    const auto t0 = std::chrono::steady_clock::now();
    {
        std::atomic<size_t> next(0);
        std::vector<std::thread> pool;
        auto work = [&] {
            for (size_t c; (c = next.fetch_add(1)) < n_chains;) {
                const Graph& graph = g->graph[c % n_contigs];
                std::vector<SampledPanel> panels(graph.size());
                for (size_t v = 0; v < panels.size(); ++v) {
                    panels[v].path_to_allele.assign(path_allele[c] + v * P, path_allele[c] + (v + 1) * P);
                    panels[v].unique_kmers = (unsigned short)(kmer_off[c][v + 1] - kmer_off[c][v]);
                }
                lines[c] = graph.sampled_panel_records(panels);
            }
        };
        if (threads <= 1) work();
        else {
            for (int t = 0; t < threads; ++t) pool.emplace_back(work);
            for (std::thread& t : pool) t.join();
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<uint64_t> line_first(n_chains + 1, 0), byte_first(n_chains + 1, 0);
    for (size_t c = 0; c < n_chains; ++c) {
        uint64_t bytes = 0;
        for (const std::string& l : lines[c]) bytes += l.size() + 1;
        line_first[c + 1] = line_first[c] + lines[c].size();
        byte_first[c + 1] = byte_first[c] + bytes;
    }
    {
        std::atomic<size_t> next(0);
        std::vector<std::thread> pool;
        auto work = [&] {
            for (size_t c; (c = next.fetch_add(1)) < n_chains;) {
                uint64_t at = byte_first[c];
                for (size_t r = 0; r < lines[c].size(); ++r) {
                    out_off[line_first[c] + r] = at;
                    memcpy(out + at, lines[c][r].data(), lines[c][r].size());
                    at += lines[c][r].size();
                    out[at++] = '\n';
                }
            }
        };
        if (threads <= 1) work();
        else {
            for (int t = 0; t < threads; ++t) pool.emplace_back(work);
            for (std::thread& t : pool) t.join();
        }
    }
    out_off[line_first.back()] = byte_first.back();
    const auto t2 = std::chrono::steady_clock::now();
    if (seconds) { seconds[0] = std::chrono::duration<double>(t1 - t0).count(); seconds[1] = std::chrono::duration<double>(t2 - t1).count(); }
    return byte_first.back();
}
