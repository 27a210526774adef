"""pangenie::genotype_cohort_sampled_reads and DeviceCountPlan::fill_device (C++ host interface over
pg_sampler_cohort_new_device and pg_sampler_counts_*): tests/cpp/test_sampled_reads.cpp, compiled the way the host tests are,
checks them on a pangenome of tools/simulate_pangenome.py against genotype_cohort_sampled over DeviceCountPlan::fill of the
same reads — every likelihood of every variant and the sampled paths, no tolerance."""
import shutil
import subprocess
import sys

import pytest

from pangenie_amd import build


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_sampled_reads"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_sampled_reads.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_sampled_reads_binary_compiles(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_sampled_reads_equal_the_host_filled_route(binary, tmp_path):
    # a pangenome of 300 kb, 600 records, 12 panel samples (24 haplotype paths: the sampler picks 7 of them and the reference
    # path), indexed by the host index builder; two samples' reads at 20x
    q = tmp_path / "q"
    sim = [sys.executable, str(build.ROOT / "tools" / "simulate_pangenome.py")]
    subprocess.run(sim + ["panel", "300000", "600", "12", "11", str(q)], check=True, stdout=subprocess.DEVNULL, timeout=300)
    reads = []
    for s, seed in enumerate((5, 6)):
        subprocess.run(sim + ["sample", str(q), "20", str(seed)], check=True, stdout=subprocess.DEVNULL, timeout=300)
        reads.append(tmp_path / f"reads{s}.fa")
        (tmp_path / "q_reads.fa").rename(reads[-1])
    subprocess.run([str(build.HOST_TEST), "index", str(q) + ".fa", str(q) + ".vcf", str(tmp_path / "idx"), "31", "0"],
                   check=True, stdout=subprocess.DEVNULL, timeout=300)
    r = subprocess.run([binary, "gpu", str(tmp_path / "idx"), str(reads[0]), str(reads[1])], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == 2
