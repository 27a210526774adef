"""Shared by the tests of the sampled panel's columns (tests/test_panel_*.py): a Python mirror of the rule of
pangenie_amd/csrc/pg_panel.h, written from the statement of the rule and checked in C++ against
Graph::sampled_panel_records by tests/cpp/test_panel_arith.cpp.  Nothing of pangenie_amd/calls.py or of the kernels is used to
form the expected values."""
import numpy as np

UNDEFINED = 0xFFFF


def rec_var_of(plan):
    return np.repeat(np.arange(plan.n_variants), np.diff(plan.rec_off.astype(np.int64)))


def mirror_text(plan, n_paths, path_allele):
    """(off [R + 1], bytes): per record the cells of the P paths joined by tabs; path_allele [V x P] allele ids"""
    pa = np.asarray(path_allele).reshape(plan.n_variants, n_paths) if plan.n_variants else np.zeros((0, n_paths), np.uint16)
    rec_var = rec_var_of(plan)
    texts = []
    for r in range(plan.n_records):
        own, vcf = plan.record(r)
        x = vcf[own[pa[rec_var[r]]]]
        texts.append("\t".join("." if int(c) == UNDEFINED else str(int(c)) for c in x).encode())
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64) if texts else np.zeros(1, np.int64)
    return off, b"".join(texts)


def mirror_uk(plan, kmer_off):
    """UK of every record: the panel's own count of its bubble"""
    return np.diff(np.asarray(kmer_off).astype(np.int64))[rec_var_of(plan)]


def cut(p, r):
    off, data = p[0], p[1]
    data = data.tobytes() if isinstance(data, np.ndarray) else data
    return data[int(off[r]):int(off[r + 1])]


def joined(prefix, uk, text):
    """(off, bytes) of the lines of a chain that is an index contig of its own: prefix (off, bytes, slot or None) with the
    decimal uk at the slot, a tab, the text, a newline"""
    lines = []
    for r in range(len(prefix[0]) - 1):
        p = cut(prefix, r)
        if len(prefix) > 2 and prefix[2] is not None:
            at = int(prefix[2][r])
            p = p[:at] + str(int(uk[r])).encode() + p[at:]
        lines.append(p + b"\t" + cut(text, r) + b"\n")
    off = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).astype(np.int64)
    return off, b"".join(lines)
