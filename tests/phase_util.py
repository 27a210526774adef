"""Shared by the tests of the phasing column (tests/test_phase_*.py): a Python mirror of the rule of pangenie_amd/csrc/pg_phase.h
(DESIGN.md 4e-9), written from the issue's statement of it and checked in C++ against the reference's stream by
tests/cpp/test_phase_arith.cpp.  Nothing of pangenie_amd/calls.py or of the kernels is used to form the expected values."""
import numpy as np

UNDEFINED = 0xFFFF
BOUND = 13   # 255|255:65535


def record_bubbles(plan):
    """(rec_var [R]: the bubble of every record, some_undefined [R]: the record has alleles of undefined sequence)"""
    rec_off = plan.rec_off.astype(np.int64)
    rec_var = np.repeat(np.arange(plan.n_variants), np.diff(rec_off))
    some = np.array([bool((plan.record(r)[1] == UNDEFINED).any()) for r in range(plan.n_records)], bool)
    return rec_var, some


def mirror_phase(plan, hap1, hap2, keyed):
    """per record (allele_1, allele_2) as an [R, 2] array; keyed [V]: the bubble's result holds likelihoods"""
    rec_var, some = record_bubbles(plan)
    out = np.zeros((plan.n_records, 2), np.int64)
    for r in range(plan.n_records):
        own, vcf = plan.record(r)
        v = int(rec_var[r])
        for i, H in enumerate((int(hap1[v]), int(hap2[v]))):
            x = int(vcf[int(own[H])])
            out[r, i] = UNDEFINED if x == UNDEFINED else 0 if (some[r] and not keyed[v]) else x
    return out


def record_text(a1, a2, kc, no_call):
    gt = "./." if no_call else "%s|%s" % ("." if a1 == UNDEFINED else a1, "." if a2 == UNDEFINED else a2)
    return ("%s:%d" % (gt, kc)).encode()


def mirror_text(phase, kc, no_call=None):
    """(off [R + 1], bytes): the packed text of R records"""
    texts = [record_text(int(p[0]), int(p[1]), int(k), bool(no_call[r]) if no_call is not None else False) for r, (p, k) in enumerate(zip(phase, kc))]
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64) if texts else np.zeros(1, np.int64)
    return off, b"".join(texts)


def as_pairs(phase):
    """a PHASE_DTYPE array as [R, 2]"""
    return np.stack([phase["allele_1"].astype(np.int64), phase["allele_2"].astype(np.int64)], axis=1) if len(phase) else np.zeros((0, 2), np.int64)


def job_mirror(job, c, plan, run_genotyping, ignore_imputed):
    """(phase [R, 2], off, bytes) of chain c from pg_job_fetch's OWN haplotypes, kept flags, n_kmers and coverage"""
    res = job.fetch(c)
    keyed = (np.asarray(res.kept) != 0) if run_genotyping else np.zeros(plan.n_variants, bool)
    phase = mirror_phase(plan, res.haplotype_1, res.haplotype_2, keyed)
    rec_var, _ = record_bubbles(plan)
    kc, uk = np.asarray(res.coverage)[rec_var], np.asarray(res.n_kmers)[rec_var]
    off, text = mirror_text(phase, kc, (uk == 0) if ignore_imputed else None)
    return phase, off, text
