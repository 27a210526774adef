"""pangenie::genotype_subsets_record_fields (the C++ host interface over pg_job_combined_record_calls + pg_job_combined_record_gl:
the reference's `-a` flow to VCF lines with no genotype bin fetched): tests/cpp/test_subsets_records.cpp, compiled the way the
host tests are, compares the lines of Graph::genotypes_records on the record fields, text for text, with the lines of the
existing overload on genotype_subsets(..., normalize = true) — on the reference's region fixture (tests/golden/
region_UniqueKmersList.cereal, index_chr1_Graph.cereal: 215 paths, two bubbles of 44 and 45 alleles, some of undefined sequence), for two
and for three subsets of the panel's paths, with and without ignore_imputed; a missing graph throws."""
import shutil
import subprocess

import pytest

from pangenie_amd import build


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_subsets_records"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_subsets_records.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_subsets_records_binary_compiles(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_the_lines_of_the_subset_flow_equal_the_lines_from_the_likelihoods(binary):
    golden = build.ROOT / "tests" / "golden"
    r = subprocess.run([binary, "gpu", str(golden / "region_UniqueKmersList.cereal"), str(golden / "index_chr1_Graph.cereal")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == 3
