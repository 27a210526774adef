// pg_phase.h — the rule of the phasing column `GT:KC` of a `-p` run, per VCF record: pg_phase_text.hip, DESIGN.md §4e-9.
//
// The reference prints it in Graph::write_phasing (src/graph.cpp:388-411) from the Viterbi haplotypes of the record's
// bubble: the bubble alleles H1, H2 folded onto the record's own alleles (Variant::separate_variants), then — for a record
// with alleles of undefined sequence — mapped onto the defined ones by GenotypingResult::get_specific_likelihoods
// (src/genotypingresult.cpp:70-96), which sets a haplotype only inside its loop over the STORED genotypes: a result that
// holds no likelihoods leaves both at 0.  Here that is two numbers per record (pg_phase) and at most 13 bytes of text.
//
// Host and device: the same functions compile into the kernels and into tests/cpp/test_phase_arith.cpp.  Every character
// goes through a sink of pg_calls.h, the decimal digits through its pgx_put_uint; no array is indexed at run time.
#pragma once
#include <stdint.h>

#include "pg_calls.h"

#ifndef PG_PHASE_DEFINED   // (the same in include/pangenie_hmm.h)
#define PG_PHASE_DEFINED
typedef struct pg_phase { uint16_t allele_1, allele_2; } pg_phase;
#define PG_PHASE_UNDEFINED 0xFFFFu   // the haplotype carries an allele of undefined sequence: printed `.`
#endif

// 255|255:65535
#define PGX_PHASE_TEXT_PER_RECORD 13u
PGX_FN uint64_t pgx_phase_text_bound(uint64_t n_records) { return PGX_PHASE_TEXT_PER_RECORD * n_records; }

// One haplotype of a record.  x = vcf_index of the record allele its bubble allele carries (0xFFFF: undefined sequence);
// some_undefined = the record has such alleles at all (the reference then asks get_specific_likelihoods); keyed = the
// bubble's result holds likelihoods, so the genotype (a, a) of every path allele's record allele a is stored.
PGX_FN uint16_t pgx_phase_allele(uint16_t x, bool some_undefined, bool keyed) {
    if (x == 0xFFFFu) return (uint16_t)PG_PHASE_UNDEFINED;
    if (some_undefined && !keyed) return 0;   // (the reference's quirk: nothing stored, nothing mapped)
    return x;
}

PGX_FN pg_phase pgx_record_phase(uint16_t x1, uint16_t x2, bool some_undefined, bool keyed) {
    pg_phase p;
    p.allele_1 = pgx_phase_allele(x1, some_undefined, keyed);
    p.allele_2 = pgx_phase_allele(x2, some_undefined, keyed);
    return p;
}

template <class Sink>
PGX_FN void pgx_phase_allele_put(uint16_t a, Sink& s) {
    if (a == PG_PHASE_UNDEFINED) s.put('.');
    else pgx_put_uint(a, s);
}

// the text of a record: `./.` for a no-call (ignore_imputed and no unique k-mers), else `a|b`; then `:` and KC
template <class Sink>
PGX_FN void pgx_phase_put(pg_phase p, uint32_t kc, bool no_call, Sink& s) {
    if (no_call) { s.put('.'); s.put('/'); s.put('.'); }
    else {
        pgx_phase_allele_put(p.allele_1, s);
        s.put('|');
        pgx_phase_allele_put(p.allele_2, s);
    }
    pgx_record_tail_put(kc, s);
}

PGX_FN uint32_t pgx_phase_text_len(pg_phase p, uint32_t kc, bool no_call) {
    pgx_count_sink s;
    s.n = 0;
    pgx_phase_put(p, kc, no_call, s);
    return s.n;
}
// writes the text to buf (PGX_PHASE_TEXT_PER_RECORD bytes suffice for alleles up to 255 and a 16-bit KC); the length
PGX_FN uint32_t pgx_phase_text(pg_phase p, uint32_t kc, bool no_call, char* buf) {
    pgx_buf_sink s;
    s.p = buf;
    s.n = 0;
    pgx_phase_put(p, kc, no_call, s);
    return s.n;
}
