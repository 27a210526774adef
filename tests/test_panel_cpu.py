"""The rule of the sampled panel's haplotype columns on the CPU (pangenie_amd/csrc/pg_panel.h): tests/cpp/test_panel_arith.cpp, a
stand-alone program, compares the bytes of pgx_panel_record_put — compiled by g++ as the kernels compile it — with
Graph::sampled_panel_records over SampledPanels, on 40 000 random bubbles of 1-4 records and 2-12 alleles with a tenth of the
ALT alleles undefined and panels of 1, 2, 16, 17 and 64 paths; then the exhaustive cell set (0, 9, 10, 99, 100, 254, undefined;
first and later cells), the bound reached by all-255 cells, Graph::sampled_panel_fixed_columns_slotted against the plain
columns and Graph::sampled_panel_records(RecordText).  Built with g++ against the host library and run; once more with the
program and the host sources it needs under the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import re
import shutil
import subprocess

from pangenie_amd import build

ROOT = build.ROOT
SRC = ROOT / "tests" / "cpp" / "test_panel_arith.cpp"
CSRC = ROOT / "pangenie_amd" / "csrc"


def run(exe, env=None):
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout, r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_the_columns_are_what_the_host_prints(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    build.build_host()
    exe = tmp_path / "test_panel_arith.bin"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{CSRC}", str(SRC), "-o", str(exe), f"-L{build.HOST_DIR}", "-lpangenie_host",
                        f"-L{CSRC}", "-lpangenie_hmm", "-lz", "-lpthread", f"-Wl,-rpath,{build.HOST_DIR}:{CSRC}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = run(exe)
    assert int(re.search(r"(\d+) checks", out).group(1)) > 400_000   # 40 000 bubbles of 1-4 records, four checks or more a record


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    build.build_hip()
    exe = tmp_path / "test_panel_arith_san.bin"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}", str(SRC),
                        str(build.HOST_DIR / "graph_io.cpp"), str(build.HOST_DIR / "pangenie_host.cpp"), "-o", str(exe), f"-L{CSRC}", "-lpangenie_hmm", "-lz",
                        "-lpthread", f"-Wl,-rpath,{CSRC}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0"))   # (the HIP runtime the library links keeps its own allocations)
