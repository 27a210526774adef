"""pangenie::genotype_cohort_sampled (C++ host interface over pg_sampler_cohort_new): tests/cpp/test_sampled_cohort.cpp,
compiled the way the host tests are, checks it per sample against HaplotypeSampler followed by HMM on objects holding that
sample's counts."""
import shutil
import subprocess

import pytest

from pangenie_amd import build


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_sampled_cohort"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_sampled_cohort.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_sampled_cohort_compiles(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_genotype_cohort_sampled_equals_sampler_then_hmm_per_sample(binary):
    r = subprocess.run([binary, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
