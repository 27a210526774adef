"""The arithmetic of the device's GL column on the CPU (pgx_gl, pgx_record_gl, pgx_gl_text of pangenie_amd/csrc/pg_calls.h):
tests/cpp/test_gl_arith.cpp, a stand-alone program, checks every value that is not deferred against what the machine's long
double prints, snprintf("%.4Lg", log10l(x)) — 10^7 random pairs (log-uniform over the whole exponent range, x in [2^-40, 1),
1 - d 2^-64 with d of every magnitude, 1 + d 2^-63), of which at most 10^-6 may be deferred; x = 1, x = 0, both sides of
2^-16300; 200 constructed boundaries d.ddd5 10^k that must be deferred, with neighbours three windows away that must not; and
every value of 100 000 random bubbles of 1-4 records against a long double std::map restatement of the host route.  Built with
g++ and run; once more under the address and undefined-behaviour sanitizers, as a program of its own (there with 10^6 random
pairs: that run looks for memory errors and undefined behaviour, the digits are the first run's).  The same header compiles
into the kernels."""
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_gl_arith.cpp"


def build_and_run(tmp_path, name, flags, n_random):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = tmp_path / name
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", *flags, f"-I{ROOT / 'pangenie_amd' / 'csrc'}", str(SRC), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(n_random)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout, r.stdout[-2000:]
    return r.stdout


def test_every_decided_value_prints_what_long_double_prints(tmp_path):
    out = build_and_run(tmp_path, "test_gl_arith.bin", ["-O2"], 10_000_000)
    n, deferred = map(int, re.search(r"random: (\d+) values, (\d+) deferred", out).groups())
    assert n == 10_000_000 and deferred <= 10   # 1e-6 of them
    values, rec_deferred = map(int, re.search(r"records: (\d+) values, (\d+) deferred", out).groups())
    assert values > 500_000 and rec_deferred <= values // 10_000
    assert int(out.strip().splitlines()[-1].split()[0]) > 10_000_000


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    build_and_run(tmp_path, "test_gl_arith_san.bin", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], 1_000_000)
