// pg_panel.h — the rule of the sample columns of the SAMPLED-PANEL VCF (the `-d` output of PanGenie, all that
// PanGenie-sampling writes), per VCF record: pg_panel_text.hip, DESIGN.md §4e-10.
//
// The reference prints it in Graph::write_sampled_panel / sample_records: one column per selected path of the reduced
// panel, FORMAT `GT`, the cell of path p = the record allele the path's bubble allele carries (Variant::separate_variants),
// as its index among the record's alleles of defined sequence, or `.` where that allele's sequence is undefined.  Here that
// is one 16-bit number per cell (pgx_panel_index) and at most 4 bytes of text: a tab in front of every cell but the first.
//
// Host and device: the same functions compile into the kernels and into tests/cpp/test_panel_arith.cpp.  Every character
// goes through a sink of pg_calls.h, the decimal digits through its pgx_put_uint; no array is indexed at run time but the
// plan's and the panel's own.
#pragma once
#include <stdint.h>

#include "pg_calls.h"

#define PGX_PANEL_UNDEFINED 0xFFFFu   // the path carries an allele of undefined sequence: printed `.`
#define PGX_PANEL_MAX_PATHS 64u       // the device's limit; the production shape is 16 or 17

// a cell is at most `255`, every cell but the first has a tab in front: R (4P - 1) for P >= 1
PGX_FN uint64_t pgx_panel_text_bound(uint64_t n_records, uint64_t n_paths) { return n_paths ? n_records * (4u * n_paths - 1u) : 0u; }

// Cell p of record r: H = the allele id of path p at the record's bubble; the record allele it carries, through the
// record's map; that allele's index among the defined ones.  map / vcf_index are the plan's arrays, m0 = map_off[r],
// v0 = vcf_off[r].
PGX_FN uint16_t pgx_panel_index(const uint16_t* map, uint32_t m0, const uint16_t* vcf_index, uint32_t v0, uint32_t H) {
    return vcf_index[v0 + map[m0 + H]];
}

// the text of a cell: a tab unless it is the record's first, then `.` or the number
template <class Sink>
PGX_FN void pgx_panel_cell_put(uint16_t x, bool first, Sink& s) {
    if (!first) s.put('\t');
    if (x == PGX_PANEL_UNDEFINED) s.put('.');
    else pgx_put_uint(x, s);
}

PGX_FN uint32_t pgx_panel_cell_len(uint16_t x, bool first) {
    pgx_count_sink s;
    s.n = 0;
    pgx_panel_cell_put(x, first, s);
    return s.n;
}

// The text of record r of a panel of P paths under a plan (rec_var, map_off, map, vcf_off, vcf_index as RecPlanDev holds
// them): the cells joined by tabs, no leading tab, no terminator.
template <class Sink>
PGX_FN void pgx_panel_record_put(const uint32_t* rec_var, const uint32_t* map_off, const uint16_t* map, const uint32_t* vcf_off, const uint16_t* vcf_index,
                                 const uint16_t* path_allele, uint32_t P, uint32_t r, Sink& s) {
    const uint64_t v = rec_var[r] & 0x7FFFFFFFu;
    for (uint32_t p = 0; p < P; ++p) pgx_panel_cell_put(pgx_panel_index(map, map_off[r], vcf_index, vcf_off[r], path_allele[v * P + p]), p == 0, s);
}

// UK of the record's line: the panel's own count of unique k-mers of the bubble (UniqueKmers::size(), in 16 bits) — not
// pg_job_fetch's rule, which answers 0 for a chain without a kept column
PGX_FN uint16_t pgx_panel_uk(const uint32_t* kmer_off, uint32_t v) { return (uint16_t)(kmer_off[v + 1] - kmer_off[v]); }
