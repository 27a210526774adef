"""pangenie::genotype_subsets and genotype_subsets_calls (the C++ host interface over pg_job_combine: the reference's `-a` flow as
one device job): tests/cpp/test_subsets.cpp, compiled the way the host tests are, checks them against one HMM(..., only_paths)
per subset, HMM::combine_likelihoods in the order of the subsets and normalize(), on tests/golden/region_UniqueKmersList.cereal —
every long double with ==, every key set, unique_kmers and coverage."""
import shutil
import subprocess

import pytest

from pangenie_amd import build


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_subsets"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_subsets.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_subsets_binary_compiles(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_subsets_equal_the_host_route(binary):
    fixture = build.ROOT / "tests" / "golden" / "region_UniqueKmersList.cereal"
    r = subprocess.run([binary, "gpu", str(fixture)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == 4
