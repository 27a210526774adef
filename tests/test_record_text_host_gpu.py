"""The VCF lines with the sample column formed as text on the device (C++ host interface: pangenie::genotype_cohort_record_text,
genotype_cohort_sampled_record_text and genotype_cohort_sampled_reads_record_text over pg_job_record_text and its packed fetch, Graph::genotypes_records(RecordText);
DESIGN.md 4e-6): tests/cpp/test_record_text_host.cpp, compiled the way the host tests are, compares whole lines, text for
text, with the lines of Graph::genotypes_records on the _record_fields siblings' output, with and without ignore_imputed — on
the reference's region fixture (215 paths, bubbles of 44 and 45 alleles: the wide records), on the demo, whose four records
carry the sample columns of tests/golden/demo/test_genotyping.vcf, and on the simulated pangenome of
tests/test_sampled_record_fields_host_gpu.py (merged bubbles, alleles of undefined sequence, two samples).  Without a device:
the splice on hand-made bytes and the refusals."""
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
    exe = tmp_path_factory.mktemp("cpp") / "test_record_text_host"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_record_text_host.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def passed(r, n_ok):
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == n_ok


def test_the_splice_on_hand_made_bytes_and_the_refusals(binary, tmp_path):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
    passed(subprocess.run([binary, "cpu"], capture_output=True, text=True, timeout=60, cwd=tmp_path), 2)


@pytest.mark.gpu
def test_the_region_fixture(binary):
    passed(subprocess.run([binary, "counted", str(GOLDEN / "region_UniqueKmersList.cereal"), str(GOLDEN / "index_chr1_Graph.cereal"), "1", "160", "80", "15"],
                          capture_output=True, text=True, timeout=300), 2)


@pytest.mark.gpu
def test_the_demo_records_carry_the_expected_sample_columns(binary, tmp_path):
    prefix = tmp_path / "preprocessing"
    r = subprocess.run([str(build.HOST_TEST), "demo-counts", str(GOLDEN / "demo"), str(prefix), "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    peak = int(r.stdout.strip().split("=")[1])
    passed(subprocess.run([binary, "counted", str(prefix) + "_counted_UniqueKmersMap.cereal", str(prefix) + "_chr1_Graph.cereal", str(peak // 4), str(peak * 4),
                           str(2 * peak), "7", str(GOLDEN / "demo" / "test_genotyping.vcf")], capture_output=True, text=True, timeout=300), 3)


@pytest.mark.gpu
def test_the_simulated_pangenome_two_samples(binary, tmp_path):
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
    passed(subprocess.run([binary, "gpu", str(tmp_path / "idx"), str(reads[0]), str(reads[1])], capture_output=True, text=True, timeout=600), 3)
