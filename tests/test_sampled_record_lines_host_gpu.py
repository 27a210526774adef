"""The VCF lines of sampled cohorts joined on the device (C++ host interface: pangenie::genotype_cohort_sampled_record_lines and
genotype_cohort_sampled_reads_record_lines over pg_job_line_prefix_strided with Graph::genotypes_fixed_columns_slotted,
pg_job_record_lines and its packed fetch): tests/cpp/test_sampled_record_lines_host.cpp, compiled the way the
host tests are, compares every sample's and chromosome's lines byte for byte with the newline-joined
Graph::genotypes_records(genotype_cohort_sampled_record_text), with and without ignore_imputed, and reads the file written by
Graph::write_genotypes(RecordLines) back — on the reference's region fixture (its counts as two samples) and on the simulated
pangenome of tests/test_record_lines_host_gpu.py with its two samples, there also from reads.  Without a device: the slotted
fixed columns with the digits of all-zero, random and 65535 counts put in at the slot equal Graph::genotypes_fixed_columns."""
import shutil
import subprocess
import sys

import pytest

from pangenie_amd import build
from tests.test_record_calls_host_gpu import leave_one_haplotype_out_of_every_seventh_record

GOLDEN = build.ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_sampled_record_lines_host"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_sampled_record_lines_host.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def passed(r, n_ok):
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == n_ok


def test_the_slotted_fixed_columns_and_the_refusals(binary, tmp_path):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
    passed(subprocess.run([binary, "cpu", str(GOLDEN / "index_chr1_Graph.cereal")], capture_output=True, text=True, timeout=120, cwd=tmp_path), 2)


@pytest.mark.gpu
def test_the_region_fixture_its_counts_as_two_samples(binary, tmp_path):
    passed(subprocess.run([binary, "counted", str(GOLDEN / "region_UniqueKmersList.cereal"), str(GOLDEN / "index_chr1_Graph.cereal"), "1", "160", "80", "15"],
                          capture_output=True, text=True, timeout=300, cwd=tmp_path), 1)


@pytest.mark.gpu
def test_the_simulated_pangenome_two_samples_from_counts_and_from_reads(binary, tmp_path):
    # the pangenome of tests/test_record_lines_host_gpu.py: 300 kb, 600 records, 12 panel samples, two samples' reads at 20x
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
    passed(subprocess.run([binary, "gpu", str(tmp_path / "idx"), str(reads[0]), str(reads[1])], capture_output=True, text=True, timeout=600, cwd=tmp_path), 2)
