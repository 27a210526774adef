"""The arithmetic of the path-subset flow on the CPU (pangenie_amd/csrc/pg_combine.h): tests/cpp/test_combine_arith.cpp, a
stand-alone program, checks a summand as the host's ldexpl reads it, the fold of one genotype key over the chains of a group
in the caller's order, the deferral rule and the walker over combined bins with pgx_decide — against this machine's x87 long
double, bit for bit.  Built with g++ and run; once more under the address and undefined-behaviour sanitizers, as a program of
its own.  The same header compiles into the kernels (pangenie_amd/csrc/pg_combine.hip)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_combine_arith.cpp"


def build_and_run(tmp_path, name, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = tmp_path / name
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", *flags, f"-I{ROOT / 'pangenie_amd' / 'csrc'}", str(SRC), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout, r.stdout[-2000:]
    return r.stdout


def test_the_fold_gives_the_bits_of_long_double(tmp_path):
    out = build_and_run(tmp_path, "test_combine_arith.bin", ["-O2"])
    assert int(out.split()[0]) > 3_000_000   # a million random keys, the deferral keys, the walker and the rest


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    build_and_run(tmp_path, "test_combine_arith_san.bin", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_without_a_device_the_unit_entry_points_answer_a_device_error_and_null_jobs_are_invalid():
    """no CPU fallback: without a device pg_combine_bins and pg_calls_from_combined answer PG_ERR_DEVICE (with one, the answer)"""
    from pangenie_amd import _lib, calls
    lib = _lib.load_hip()
    aoff = np.array([0, 2], np.uint32)
    chains = dict(kept=[[1], [1]], allele_present=[[1, 1], [1, 0]], lik=[[0.5, 0.5, 0.75], [0.5, 0.5, 0.5]], lik_exp=[[-3, -9, -1], [-3, 0, 0]])
    bins = np.zeros(3, calls.COMBINED_DTYPE)
    bins["flags"] = calls.PG_COMBINED_PRESENT
    bins["m"], bins["e"] = [1 << 63, 1 << 63, 3 << 62], [-67, -73, -65]   # 2^-4, 2^-10, 0.375
    if lib.pg_hmm_device_count() > 0:
        got = calls.combine_bins(aoff, **chains)
        assert [int(f) for f in got["flags"]] == [1, 1, 1]
        assert list(calls.combined_to_longdouble(got)) == [np.longdouble(2.0) ** -3, np.longdouble(2.0) ** -10, np.longdouble(0.375)]
        rec = calls.calls_from_combined(aoff, [0, 1], bins)[0]
        assert (int(rec["allele_1"]), int(rec["allele_2"]), int(rec["flags"])) == (1, 1, calls.PG_CALL_OK)
    else:
        from pangenie_amd.hmm import PanGenieError
        with pytest.raises(PanGenieError) as e:
            calls.combine_bins(aoff, **chains)
        assert e.value.code == _lib.PG_ERR_DEVICE
        with pytest.raises(PanGenieError) as e:
            calls.calls_from_combined(aoff, [0, 1], bins)
        assert e.value.code == _lib.PG_ERR_DEVICE
    # what is no pg_combined_bin is refused before any device is asked for
    bad = bins.copy()
    bad["m"][1] = 5
    with pytest.raises(Exception) as e:
        calls.calls_from_combined(aoff, [0, 1], bad)
    assert e.value.code == _lib.PG_ERR_INVALID
    # a null job is refused before any device is asked for
    err = C.create_string_buffer(64)
    assert lib.pg_job_combine_plan(None, 0, None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_combine(None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_combined_calls(None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined(None, 0, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined_all(None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined_calls(None, 0, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_combined_calls_all(None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_combined(None, 0, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_combined_calls(None, 0, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_n_groups(None) == 0
    assert lib.pg_job_combine_ms(None) == 0.0 and lib.pg_job_combined_calls_ms(None) == 0.0
