"""CPU-only checks of the device-resident entry of the sampled cohort (include/pangenie_sampler.h: pg_sampler_counts_* and
pg_sampler_cohort_new_device): the symbols are exported and listed, and everything the host can decide — null arguments, an
empty shape, a sample outside the handle — is refused with its message before any device call (this machine may have no
GPU)."""
import ctypes as C

import pytest

from pangenie_amd import _lib, build
from pangenie_amd import sampler as smp

NEW_SYMBOLS = ("pg_sampler_counts_new", "pg_sampler_counts_destroy", "pg_sampler_counts_rows", "pg_sampler_cohort_new_device")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return smp._hip()


def test_the_four_symbols_are_exported_and_listed(lib):
    for sym in NEW_SYMBOLS:
        assert sym in smp.SAMPLER_ABI_SYMBOLS, sym
        assert hasattr(lib, sym), sym
    header = (build.ROOT / "include" / "pangenie_sampler.h").read_text()
    for sym in NEW_SYMBOLS:
        assert sym + "(" in header, sym


def test_null_arguments_are_invalid_without_a_device(lib):
    err = C.create_string_buffer(512)
    h = C.c_void_p(1)
    nk, nv = (C.c_uint64 * 2)(5, 0), (C.c_uint32 * 2)(2, 0)
    assert lib.pg_sampler_counts_new(0, 2, None, nv, 1, C.byref(h), err, 512) == _lib.PG_ERR_INVALID
    assert b"pg_sampler_counts_new: null argument" in err.value and not h.value
    assert lib.pg_sampler_counts_new(0, 2, nk, None, 1, C.byref(h), err, 512) == _lib.PG_ERR_INVALID
    assert lib.pg_sampler_counts_new(0, 2, nk, nv, 1, None, err, 512) == _lib.PG_ERR_INVALID
    assert lib.pg_sampler_counts_new(0, 0, nk, nv, 1, C.byref(h), err, 512) == _lib.PG_ERR_INVALID and b"no contigs" in err.value
    assert lib.pg_sampler_counts_new(0, 2, nk, nv, 0, C.byref(h), err, 512) == _lib.PG_ERR_INVALID and b"no samples" in err.value
    assert lib.pg_sampler_counts_new(0, 2, nk, nv, 0, C.byref(h), None, 0) == _lib.PG_ERR_INVALID   # (no room for a message)
    pk, pc = C.POINTER(_lib.u16p)(), C.POINTER(_lib.u16p)()
    assert lib.pg_sampler_counts_rows(None, 0, C.byref(pk), C.byref(pc), err, 512) == _lib.PG_ERR_INVALID
    assert b"pg_sampler_counts_rows: null handle" in err.value and not pk and not pc
    assert lib.pg_sampler_counts_destroy(None) == _lib.PG_OK
    # the cohort entry: each pointer in turn, none of them reaching a device call
    job = C.c_void_p(1)
    one = C.c_void_p(8)   # (never dereferenced: another argument is null)
    ld = C.c_longdouble(25000.0)
    call = lambda index, samples, table, params, out: lib.pg_sampler_cohort_new_device(
        0, 1, C.cast(index, C.POINTER(_lib.PgContigBatch)), 1, C.cast(samples, C.POINTER(_lib.PgSampleCounts)), 3, 0, 1.26, ld, 10,
        table, params, None, None, out, err, 512)
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        job.value = 1
        assert call(*args, C.byref(job)) == _lib.PG_ERR_INVALID
        assert b"pg_sampler_cohort_new_device: null argument" in err.value and not job.value
    assert call(one, one, one, one, None) == _lib.PG_ERR_INVALID


def test_counts_new_without_a_device_is_a_device_error(lib):
    if lib.pg_hmm_device_count() != 0:
        return   # (with a device the same call succeeds: tests/test_sampled_cohort_device_gpu.py)
    err = C.create_string_buffer(512)
    h = C.c_void_p(1)
    nk, nv = (C.c_uint64 * 2)(5, 0), (C.c_uint32 * 2)(2, 0)
    assert lib.pg_sampler_counts_new(0, 2, nk, nv, 3, C.byref(h), err, 512) == _lib.PG_ERR_DEVICE
    assert b"no HIP device" in err.value and not h.value
    with pytest.raises(Exception) as e:
        smp.SamplerCounts([], 1)
    assert getattr(e.value, "code", None) == _lib.PG_ERR_INVALID   # no contigs: decided before the device is asked for
