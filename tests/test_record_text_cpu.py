"""The rule of the record text on the CPU (pgx_record_text, pgx_record_text_len, pgx_record_text_bound of
pangenie_amd/csrc/pg_calls.h): tests/cpp/test_record_text_arith.cpp, a stand-alone program, compares the bytes with a
restatement of what the host's ostringstream prints of the same fields — on the exhaustive value sets of
tests/test_record_text_values_gpu.py, under every call flag, with and without no_call — checks that the length is the written
length, that the records left to the host have none, and that the bound is never exceeded and is reached.  Built with g++ and
run; once more under the address and undefined-behaviour sanitizers, as a program of its own.  The same header compiles into
the kernels."""
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_record_text_arith.cpp"


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


def test_the_text_is_what_the_host_stream_prints(tmp_path):
    out = build_and_run(tmp_path, "test_record_text_arith.bin", ["-O2"])
    assert int(re.search(r"(\d+) checks", out).group(1)) > 200_000   # 37 062 records of three values, twice, three checks or more each


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    build_and_run(tmp_path, "test_record_text_arith_san.bin", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
