"""CPU-only checks of include/pangenie_counts.h (the count plan): every declared symbol is exported and listed
by the Python view, null arguments are refused before any device call (this machine may have no GPU), and the parsing half
of CountPlan.from_tables gives the offsets and codes of the table's own strings."""
import ctypes as C
import gzip
import re
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import _lib, build, kmers

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return kmers._counts()


def test_every_declared_symbol_is_exported(lib):
    header = (ROOT / "include" / "pangenie_counts.h").read_text()
    declared = set(re.findall(r"\b(pg_count_plan_[a-z_]+)\s*\(", header))
    assert declared == set(kmers.COUNTS_ABI_SYMBOLS) and len(declared) == 7
    for sym in kmers.COUNTS_ABI_SYMBOLS:
        assert hasattr(lib, sym), sym
    # the older headers keep their own lists: nothing of the plan is declared there
    for other in ("pangenie_hmm.h", "pangenie_sampler.h", "pangenie_kmers.h"):
        assert "pg_count_plan" not in (ROOT / "include" / other).read_text()
    # the seam between pg_kmers.hip and pg_shim.cpp is internal: not exported
    assert not hasattr(lib, "pgi_job_fill_begin") and not hasattr(lib, "pgi_job_fill_end")


def test_null_counter_and_null_out_are_invalid_without_a_device(lib):
    h = C.c_void_p(1)
    assert lib.pg_count_plan_new(None, 0, None, 0, C.byref(h)) == _lib.PG_ERR_INVALID
    assert not h.value and b"null counter" in lib.pg_kmer_last_error()
    assert lib.pg_count_plan_new(None, 0, None, 0, None) == _lib.PG_ERR_INVALID
    assert b"null out" in lib.pg_kmer_last_error()
    assert lib.pg_count_plan_fill_host(None, 1, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_count_plan_fill_device(None, 1, None, None) == _lib.PG_ERR_INVALID
    err = C.create_string_buffer(256)
    assert lib.pg_count_plan_fill_job(None, 1, None, 0, err, 256) == _lib.PG_ERR_INVALID and b"null plan" in err.value
    assert lib.pg_count_plan_stats(None, None, None, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_count_plan_destroy(None) == _lib.PG_OK
    assert lib.pg_count_plan_last_fill_ms(None) == 0.0


def rows_of(path):
    """the data rows of a table, split by hand: (chromosome, start, unique k-mers, flanking k-mers)"""
    out = []
    with gzip.open(path, "rt") as f:
        for line in f:
            cols = line.rstrip("\n").split("\t")
            if cols[0].startswith("#"):
                continue
            lists = [[] if c == "nan" else c.split(",") for c in cols[3:5]]
            out.append((cols[0], int(cols[1]), lists[0], lists[1]))
    return out


def check_table(path, k):
    rows = rows_of(path)
    got = kmers.parse_kmer_table(path, k)
    assert got.n_variants == len(rows) and got.chromosome == rows[0][0]
    assert got.kmer_off.dtype == np.uint32 and got.flank_off.dtype == np.uint64 and got.kmer_code.dtype == np.uint64
    assert got.start.tolist() == [r[1] for r in rows]
    assert got.kmer_off.tolist() == np.cumsum([0] + [len(r[2]) for r in rows]).tolist()
    assert got.flank_off.tolist() == np.cumsum([0] + [len(r[3]) for r in rows]).tolist()
    assert np.array_equal(got.kmer_code, kmers.canonical_codes([s for r in rows for s in r[2]], k))
    assert np.array_equal(got.flank_code, kmers.canonical_codes([s for r in rows for s in r[3]], k))
    return got


def test_parsing_half_on_the_golden_table():
    got = check_table(GOLDEN / "index_chr1_kmers.tsv.gz", 31)
    assert got.n_variants == 2 and got.kmer_code.size > 0 and got.flank_code.size > 0
    assert (got.kmer_code != kmers.NOT_REGISTERED).all()


def test_parsing_half_on_a_table_with_nan_columns_and_an_n(tmp_path):
    path = tmp_path / "t_chrZ_kmers.tsv.gz"
    with gzip.open(path, "wt") as f:
        f.write("#chromosome\tstart\tend\tunique_kmers\tunique_kmers_overhang\n")
        f.write("chrZ\t10\t11\tACGTA,CCCCC\tGGGGG,TTTTA,ACGTN\n")
        f.write("chrZ\t20\t21\tnan\tAAAAA\n")
        f.write("chrZ\t30\t31\tACNTA\tnan\n")
        f.write("chrZ\t40\t41\tnan\tnan\n")
    got = check_table(path, 5)
    assert got.kmer_off.tolist() == [0, 2, 2, 3, 3] and got.flank_off.tolist() == [0, 3, 4, 4, 4]
    assert got.kmer_code[2] == kmers.NOT_REGISTERED and got.flank_code[2] == kmers.NOT_REGISTERED
    assert got.kmer_code[1] == kmers.canonical_codes(["GGGGG"], 5)[0]   # CCCCC under its reverse complement
    with pytest.raises(ValueError):
        kmers.parse_kmer_table(path, 4)
