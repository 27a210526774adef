"""GT, GQ and GL per VCF record from combined bins, the arithmetic on the CPU (pangenie_amd/csrc/pg_combine.h, pg_calls.h):
tests/cpp/test_combined_records_arith.cpp, a stand-alone program, takes the route of pg_combine_records.hip — pgc_fold per key
over the chains, the key walk over the combined bins, pgx_decide_record and pgx_record_gl — and compares it with this machine's
x87 long double: std::map sums in group order, normalise, fold, specific likelihoods, likeliest genotype, quality and the
digits of log10l.  Built with g++ and run; once more, on fewer random bubbles, under the address and undefined-behaviour
sanitizers, as a program of its own.  The same headers compile into the kernels."""
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_combined_records_arith.cpp"


def build_and_run(tmp_path, name, flags, args=()):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = tmp_path / name
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", *flags, f"-I{ROOT / 'pangenie_amd' / 'csrc'}", str(SRC), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout, r.stdout[-2000:]
    return r.stdout


def test_records_from_combined_bins_give_what_long_double_gives(tmp_path):
    out = build_and_run(tmp_path, "test_combined_records_arith.bin", ["-O2"])
    m = re.search(r"(\d+) records \((\d+) deferred\), (\d+) GL values \((\d+) deferred\)", out)
    assert m, out[-500:]
    records, values = int(m.group(1)), int(m.group(3))
    assert records > 350_000 and values > 1_500_000   # 200 000 random bubbles of 1 .. 3 records, and the constructed cases


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    build_and_run(tmp_path, "test_combined_records_arith_san.bin", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                  ["20000"])
