// test_panel_arith.cpp — the rule of the sampled panel's haplotype columns (pangenie_amd/csrc/pg_panel.h: pgx_panel_index,
// pgx_panel_cell_put / _len, pgx_panel_record_put, pgx_panel_uk, pgx_panel_text_bound), compiled by g++ as the kernels compile
// it, against Graph::sampled_panel_records over SampledPanels (pangenie_amd/host/graph_io.cpp: Variant::records with a sampled
// panel, the ostringstream of sample_records), byte for byte: random bubbles of 1-4 records, 2-12 alleles, a tenth of the ALT
// alleles of undefined sequence, panels of 1, 2, 16, 17 and 64 paths; then the exhaustive cell set; then
// Graph::sampled_panel_fixed_columns_slotted against the plain columns and Graph::sampled_panel_records(RecordText).
// No device: links the host library's sources.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../pangenie_amd/host/graph_io.hpp"
#include "pg_panel.h"

using namespace pangenie;

static long n_checked = 0, n_failed = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        ++n_checked;                                              \
        if (!(cond)) {                                            \
            if (++n_failed <= 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                         \
    } while (0)

// a distinct ALT sequence per number; `undefined`: with a base outside ACGT
static std::string alt_sequence(unsigned i, bool undefined) {
    std::string s = "C";
    for (int k = 0; k < 3; ++k) { s += "ACGT"[i % 4]; i /= 4; }
    if (undefined) s += 'N';
    return s;
}

int main() {
    std::mt19937 rng(41017);
    auto below = [&](unsigned n) { return (unsigned)(rng() % n); };
    const unsigned path_counts[5] = {1, 2, 16, 17, 64};
    long n_bubbles = 0, n_undefined_cells = 0, n_combined = 0, n_two_digit = 0;
    for (int g = 0; g < 800; ++g) {
        const unsigned P = path_counts[g % 5], V = 50;
        std::vector<Variant> variants;
        std::vector<std::vector<std::string>> ids;
        std::vector<unsigned> n_alleles_of(V);
        size_t start = 10;
        for (unsigned v = 0; v < V; ++v) {
            const unsigned n_alleles = 2 + below(11), n_records = 1 + below(4);   // bubble alleles 2 .. 12, records 1 .. 4
            const bool combined = n_records > 1;
            n_alleles_of[v] = n_alleles;
            std::vector<std::vector<std::string>> records(n_records);
            std::vector<std::vector<unsigned short>> combinations(n_alleles, std::vector<unsigned short>(n_records, 0));
            for (unsigned j = 0; j < n_records; ++j) {
                const unsigned nA = combined ? 2 + below(n_alleles < 6 ? n_alleles - 1 : 5) : n_alleles;
                records[j].push_back("A");
                for (unsigned a = 1; a < nA; ++a) records[j].push_back(alt_sequence(a, below(10) == 0));
                for (unsigned a = 1; a < n_alleles; ++a) combinations[a][j] = (unsigned short)(combined ? below(nA) : a);
                ids.push_back({});
            }
            std::vector<unsigned short> paths(5);   // the panel's own paths (AF): any bubble alleles
            for (unsigned short& a : paths) a = (unsigned short)below(n_alleles);
            variants.push_back(Variant::from_parts("chrT", start, "ACGT", "TGCA", records, std::vector<std::string>(n_records - 1, "GT"), combinations, paths, false));
            start = variants.back().get_end_position() + 40;
            n_combined += combined;
        }
        const Graph graph = Graph::from_parts("chrT", 4, false, variants, ids);
        const RecordPlan plan = graph.record_plan();
        const size_t R = plan.nr_of_records();
        std::vector<uint32_t> rec_var(R), kmer_off(V + 1, 0);
        for (unsigned v = 0; v < V; ++v)
            for (uint32_t q = plan.rec_off[v]; q < plan.rec_off[v + 1]; ++q) rec_var[q] = v | (below(2) ? 0x80000000u : 0u);   // (bit 31 is not the rule's)
        std::vector<uint16_t> path_allele((size_t)V * P);
        std::vector<SampledPanel> panels(V);
        std::vector<unsigned short> uk(V);
        for (unsigned v = 0; v < V; ++v) {
            for (unsigned p = 0; p < P; ++p) path_allele[(size_t)v * P + p] = (uint16_t)below(n_alleles_of[v]);
            panels[v].path_to_allele.assign(path_allele.begin() + (size_t)v * P, path_allele.begin() + (size_t)(v + 1) * P);
            uk[v] = (unsigned short)(below(4) ? below(300) : below(65536));
            panels[v].unique_kmers = uk[v];
            kmer_off[v + 1] = kmer_off[v] + uk[v];
        }
        n_bubbles += V;
        const std::vector<std::string> want = graph.sampled_panel_records(panels);
        const std::vector<std::string> fixed = graph.sampled_panel_fixed_columns(uk);
        CHECK(want.size() == R && fixed.size() == R, "%zu lines, %zu fixed columns, %zu records", want.size(), fixed.size(), R);
        if (want.size() != R || fixed.size() != R) continue;
        RecordText text;
        text.off.assign(R + 1, 0);
        text.unique_kmers = uk;
        for (size_t r = 0; r < R; ++r) {
            std::vector<char> buf(pgx_panel_text_bound(1, P) + 8, '#');
            pgx_buf_sink s;
            s.p = buf.data(); s.n = 0;
            pgx_panel_record_put(rec_var.data(), plan.map_off.data(), plan.map.data(), plan.vcf_off.data(), plan.vcf_index.data(), path_allele.data(), P, (uint32_t)r, s);
            uint32_t len = 0;
            const uint32_t v = rec_var[r] & 0x7FFFFFFFu;
            for (unsigned p = 0; p < P; ++p) {
                const uint16_t x = pgx_panel_index(plan.map.data(), plan.map_off[r], plan.vcf_index.data(), plan.vcf_off[r], path_allele[(size_t)v * P + p]);
                len += pgx_panel_cell_len(x, p == 0);
                n_undefined_cells += x == PGX_PANEL_UNDEFINED;
                n_two_digit += x != PGX_PANEL_UNDEFINED && x >= 10;
            }
            CHECK(len == s.n, "record %zu: length %u, written %u", r, len, s.n);
            CHECK(s.n <= pgx_panel_text_bound(1, P) && buf[s.n] == '#', "record %zu: %u bytes, bound %llu", r, s.n, (unsigned long long)pgx_panel_text_bound(1, P));
            const std::string got = fixed[r] + '\t' + std::string(buf.data(), s.n);
            CHECK(got == want[r], "graph %d record %zu: got '%s' want '%s'", g, r, got.c_str(), want[r].c_str());
            CHECK(pgx_panel_uk(kmer_off.data(), v) == uk[v], "UK of bubble %u", v);
            text.bytes.append(buf.data(), s.n);
            text.off[r + 1] = text.bytes.size();
        }
        // the columns arriving as bytes: the same lines
        CHECK(graph.sampled_panel_records(text) == want, "graph %d: Graph::sampled_panel_records(RecordText) differs", g);
        // the slotted columns: the plain ones with the digits of UK taken out at the slot
        std::vector<uint32_t> slot;
        const std::vector<std::string> slotted = graph.sampled_panel_fixed_columns_slotted(&slot);
        CHECK(slotted.size() == R && slot.size() == R, "%zu slotted columns, %zu slots", slotted.size(), slot.size());
        for (size_t r = 0; r < R && r < slotted.size() && r < slot.size(); ++r) {
            std::string with = slotted[r];
            CHECK(slot[r] <= with.size() && slot[r] >= 4 && with.compare(slot[r] - 4, 4, ";UK=") == 0, "record %zu: slot %u", r, slot[r]);
            with.insert(slot[r], std::to_string(uk[rec_var[r] & 0x7FFFFFFFu]));
            CHECK(with == fixed[r], "record %zu: slotted '%s' plain '%s'", r, with.c_str(), fixed[r].c_str());
            CHECK(with.size() >= 3 && with.compare(with.size() - 3, 3, "\tGT") == 0, "record %zu ends in '%s'", r, with.c_str());
        }
    }
    CHECK(n_bubbles == 40000 && n_undefined_cells > 1000 && n_combined > 10000 && n_two_digit > 1000, "the random bubbles miss a case: %ld %ld %ld %ld", n_bubbles,
          n_undefined_cells, n_combined, n_two_digit);

    // the exhaustive cell set
    const unsigned values[7] = {0, 9, 10, 99, 100, 254, 0xFFFF};
    for (unsigned x : values)
        for (int first = 0; first < 2; ++first) {
            char buf[16];
            memset(buf, '#', sizeof(buf));
            pgx_buf_sink s;
            s.p = buf; s.n = 0;
            pgx_panel_cell_put((uint16_t)x, first != 0, s);
            const std::string want = std::string(first ? "" : "\t") + (x == 0xFFFF ? std::string(".") : std::to_string(x));
            CHECK(std::string(buf, s.n) == want && buf[s.n] == '#', "cell %u: got '%.*s' want '%s'", x, (int)s.n, buf, want.c_str());
            CHECK(pgx_panel_cell_len((uint16_t)x, first != 0) == want.size(), "cell %u: length", x);
            CHECK(want.size() <= 4, "a cell of %zu bytes", want.size());
        }
    // the bound: P cells of `255` and P - 1 tabs; reached by nothing shorter
    CHECK(pgx_panel_text_bound(0, 5) == 0 && pgx_panel_text_bound(5, 0) == 0 && pgx_panel_text_bound(1, 1) == 3 && pgx_panel_text_bound(7, 17) == 7u * 67u &&
              pgx_panel_text_bound(1ull << 31, 64) == (1ull << 31) * 255ull,
          "bound");
    {
        const uint32_t rec_var[1] = {0}, map_off[2] = {0, 1}, vcf_off[2] = {0, 1};
        const uint16_t map[1] = {0}, vcf_index[1] = {255}, pa[64] = {0};   // (no plan holds 255: the bound's own case)
        for (unsigned P : path_counts) {
            std::vector<char> buf(pgx_panel_text_bound(1, P) + 1, '#');
            pgx_buf_sink s;
            s.p = buf.data(); s.n = 0;
            pgx_panel_record_put(rec_var, map_off, map, vcf_off, vcf_index, pa, P, 0, s);
            CHECK(s.n == pgx_panel_text_bound(1, P) && buf[s.n] == '#', "P = %u: %u bytes of all-255 cells, bound %llu", P, s.n, (unsigned long long)pgx_panel_text_bound(1, P));
        }
    }
    printf("%ld checks, %ld failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
