"""The VCF lines of a SAMPLED cohort from the device's record fields (C++ host interface:
pangenie::genotype_cohort_sampled_record_fields and genotype_cohort_sampled_reads_record_fields over
pg_job_record_plan_strided, pg_job_record_calls, pg_job_record_gl and the packed fetches):
tests/cpp/test_sampled_record_fields.cpp, compiled the way the host tests are, compares whole lines, text for text, with the
lines of the existing overload on genotype_cohort_sampled's / genotype_cohort_sampled_reads' normalised results, and the
sampled paths — on the simulated pangenome of tests/test_sampled_reads_host_gpu.py (24 paths, the sampler picks 7 and the
reference path) with merged bubbles and alleles of undefined sequence, two samples, with and without ignore_imputed.  Without
a device: the refusals that need no job."""
import shutil
import subprocess
import sys

import pytest

from pangenie_amd import build
from tests.test_record_calls_host_gpu import leave_one_haplotype_out_of_every_seventh_record


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_sampled_record_fields"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_sampled_record_fields.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_the_refusals_that_need_no_job(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
    r = subprocess.run([binary, "cpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == 1


@pytest.mark.gpu
def test_the_lines_of_a_sampled_cohort_from_the_record_fields_equal_the_lines_from_the_likelihoods(binary, tmp_path):
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
    assert leave_one_haplotype_out_of_every_seventh_record(tmp_path / "q.vcf") >= 30
    subprocess.run([str(build.HOST_TEST), "index", str(q) + ".fa", str(q) + ".vcf", str(tmp_path / "idx"), "31", "0"],
                   check=True, stdout=subprocess.DEVNULL, timeout=300)
    r = subprocess.run([binary, "gpu", str(tmp_path / "idx"), str(reads[0]), str(reads[1])], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == 2
