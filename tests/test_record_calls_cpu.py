"""The arithmetic of the device's calls per VCF record on the CPU (pgx_decide_record, pangenie_amd/csrc/pg_calls.h):
tests/cpp/test_record_calls_arith.cpp, a stand-alone program, runs it against a long double restatement of the host route —
normalise the bubble, fold it onto the record's alleles in a std::map, drop the undefined alleles and renormalise, likeliest
genotype, quality — on 220 000 random bubbles of 1-4 records and on the constructed cases of tests/test_record_calls_edges_gpu.py.
Built with g++ and run; once more under the address and undefined-behaviour sanitizers, as a program of its own.  The same
header compiles into the kernels, so what passes here is what k_rcalls computes with."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_record_calls_arith.cpp"


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


def test_record_decisions_give_what_long_double_gives(tmp_path):
    out = build_and_run(tmp_path, "test_record_calls_arith.bin", ["-O2"])
    assert int(out.split()[0]) > 400_000   # 220 000 random bubbles with 2.5 records on average, and the constructed cases


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    build_and_run(tmp_path, "test_record_calls_arith_san.bin", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
