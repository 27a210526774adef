"""Multi-sample VCF lines joined on the device (C++ host interface: pangenie::genotype_cohort_record_lines over
pg_job_line_prefix, pg_job_record_lines and its packed fetch; Graph::genotypes_fixed_columns, compose_record_lines,
Graph::write_genotypes(RecordLines)): tests/cpp/test_record_lines_host.cpp, compiled the way the host tests
are, splits every line at tabs and compares columns 1-9 and column 9 + s with the single-sample lines of
Graph::genotypes_records(genotype_cohort_record_text), with and without ignore_imputed, and reads the written file back — on
the reference's region fixture (one sample, and the same counts as two samples) and on the simulated pangenome of
tests/test_record_text_host_gpu.py with its two samples.  Without a device: the fixed columns against whole lines on the
region fixture's graph, the multi-sample header, the host's composition of a line the device left out, the file."""
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
    exe = tmp_path_factory.mktemp("cpp") / "test_record_lines_host"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_record_lines_host.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def passed(r, n_ok):
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == n_ok


def test_the_fixed_columns_the_header_the_composition_and_the_file(binary, tmp_path):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
    passed(subprocess.run([binary, "cpu", str(GOLDEN / "index_chr1_Graph.cereal")], capture_output=True, text=True, timeout=120, cwd=tmp_path), 5)


@pytest.mark.gpu
def test_the_region_fixture_one_sample_and_the_same_counts_twice(binary, tmp_path):
    passed(subprocess.run([binary, "counted", str(GOLDEN / "region_UniqueKmersList.cereal"), str(GOLDEN / "index_chr1_Graph.cereal"), "1", "160", "80"],
                          capture_output=True, text=True, timeout=300, cwd=tmp_path), 2)


@pytest.mark.gpu
def test_the_simulated_pangenome_two_samples(binary, tmp_path):
    # the pangenome of tests/test_record_text_host_gpu.py: 300 kb, 600 records, 12 panel samples, two samples' reads at 20x
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
    passed(subprocess.run([binary, "gpu", str(tmp_path / "idx"), str(reads[0]), str(reads[1])], capture_output=True, text=True, timeout=600, cwd=tmp_path), 1)
