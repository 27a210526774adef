"""The arithmetic of the device's genotype calls on the CPU (pangenie_amd/csrc/pg_calls.h): tests/cpp/test_calls_arith.cpp, a
stand-alone program, checks every operation of the integer pairs — add, sub, div, compare, the conversion of a bin, 1 - x, the
genotype-quality table, the whole decision — against this machine's x87 long double, bit for bit.  Built with g++ and run; once
more under the address and undefined-behaviour sanitizers, as a program of its own.  The same header compiles into the kernels
(pangenie_amd/csrc/pg_calls.hip), so what passes here is what the device computes with."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_calls_arith.cpp"


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


def test_integer_pairs_give_the_bits_of_long_double(tmp_path):
    out = build_and_run(tmp_path, "test_calls_arith.bin", ["-O2"])
    assert int(out.split()[0]) > 5_000_000   # a million random operand pairs, eight checks each, and the rest


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    build_and_run(tmp_path, "test_calls_arith_san.bin", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_calls_from_bins_without_a_device_is_a_device_error_not_a_host_answer():
    """no CPU fallback: without a device the unit entry point answers PG_ERR_DEVICE (with one it answers the call)"""
    from pangenie_amd import _lib, calls
    lib = _lib.load_hip()
    arrays = (np.array([0, 2], np.uint32), [0, 1], [1], [1, 1], [0.5, 0.5, 0.75], [-3, -9, -1])
    if lib.pg_hmm_device_count() > 0:
        rec = calls.calls_from_bins(*arrays)[0]
        assert (int(rec["allele_1"]), int(rec["allele_2"]), int(rec["flags"])) == (1, 1, calls.PG_CALL_OK)
    else:
        from pangenie_amd.hmm import PanGenieError
        with pytest.raises(PanGenieError) as e:
            calls.calls_from_bins(*arrays)
        assert e.value.code == _lib.PG_ERR_DEVICE
    # a null job is refused before any device is asked for
    err = C.create_string_buffer(64)
    assert lib.pg_job_calls(None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_calls(None, 0, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_fetch_calls_all(None, None, err, 64) == _lib.PG_ERR_INVALID
    assert lib.pg_job_device_calls(None, 0, None, None) == _lib.PG_ERR_INVALID
    assert lib.pg_job_calls_ms(None) == 0.0
