"""CPU-only checks of include/pangenie_kmers.h: the library exports every symbol the header declares and the Python view
lists, and the k-mer size is refused before any device call (this machine may have no GPU)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from pangenie_amd import _lib, build, kmers

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return kmers._hip()


def test_every_declared_symbol_is_exported(lib):
    header = (ROOT / "include" / "pangenie_kmers.h").read_text()
    declared = set(re.findall(r"\b(pg_kmer_[a-z_]+)\s*\(", header))
    assert declared == set(kmers.KMERS_ABI_SYMBOLS)
    for sym in kmers.KMERS_ABI_SYMBOLS:
        assert hasattr(lib, sym), sym


@pytest.mark.parametrize("k", [0, 33, 64, 2 ** 32 - 1])
def test_kmer_size_outside_1_to_32_is_invalid_without_a_device(lib, k):
    h = C.c_void_p(1)
    assert lib.pg_kmer_counter_new(k, 0, C.byref(h)) == _lib.PG_ERR_INVALID
    assert not h.value
    assert b"1..32" in lib.pg_kmer_last_error()
    with pytest.raises(kmers.KmerCounterError) as e:
        kmers.KmerCounter(k)
    assert e.value.code == _lib.PG_ERR_INVALID


def test_null_out_is_invalid(lib):
    assert lib.pg_kmer_counter_new(31, 0, None) == _lib.PG_ERR_INVALID


def test_tile_is_a_whole_number_of_16_byte_chunks(lib):
    assert kmers.tile_bytes() > 0 and kmers.tile_bytes() % 16 == 0


def test_canonical_codes_helper():
    # ACGT is its own reverse complement; CGTA / TACG are one class; first letter in the highest bits
    got = kmers.canonical_codes(["ACGT", "CGTA", "TACG", "acgt", "TTTT", "ACGN"], 4)
    assert got[0] == 0b00011011 and got[1] == got[2] and got[3] == got[0] and got[4] == 0
    assert got[5] == kmers.NOT_REGISTERED
    assert kmers.canonical_codes(["T" * 32], 32)[0] == 0 and kmers.canonical_codes(["G" * 32], 32)[0] == int("01" * 32, 2)
    assert kmers.canonical_codes([], 5).dtype == np.uint64
    with pytest.raises(ValueError):
        kmers.canonical_codes(["ACG"], 4)
