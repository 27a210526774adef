"""The rule of the phasing column on the CPU (pgx_record_phase, pgx_phase_text, pgx_phase_text_len, pgx_phase_text_bound of
pangenie_amd/csrc/pg_phase.h): tests/cpp/test_phase_arith.cpp, a stand-alone program, compares the bytes with a restatement of
the stream the reference sends a bubble's result through — a GenotypingResult with and without stored likelihoods, folded per
record, get_specific_likelihoods over the defined alleles, phased_field's ostringstream — on random bubbles of 1-4 records and
2-12 alleles with undefined alleles, haplotypes on defined and undefined alleles, keyed and not, ignore_imputed with UK 0 and
non-zero; then the exhaustive format set.  The length is the written length, the bound is never exceeded and is reached.  Built
with g++ and run; once more under the address and undefined-behaviour sanitizers, as a program of its own.  The same header
compiles into the kernels."""
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_phase_arith.cpp"


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


def test_the_column_is_what_the_reference_stream_prints(tmp_path):
    out = build_and_run(tmp_path, "test_phase_arith.bin", ["-O2"])
    assert int(re.search(r"(\d+) checks", out).group(1)) > 400_000   # 40 000 bubbles of 1-4 records, four checks or more each


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    build_and_run(tmp_path, "test_phase_arith_san.bin", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
