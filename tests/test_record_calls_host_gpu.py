"""pangenie::genotype_cohort_record_calls (C++ host interface over pg_job_record_plan / pg_job_record_calls):
tests/cpp/test_record_calls_host.cpp, compiled the way the host tests are, checks it against the VCF text itself —
genotype_cohort, normalize, Graph::genotypes_records — on a pangenome of tools/simulate_pangenome.py with two samples: the
GT and GQ of every record line's sample column, with and without ignore_imputed, no tolerance.  The pangenome's records lie
close enough for the index builder to merge some into one bubble; one panel haplotype of every seventh record is left out
(`.`), which the index builder turns into an allele of undefined sequence (the program asserts that both exist)."""
import shutil
import subprocess
import sys

import pytest

from pangenie_amd import build


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_record_calls_host"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_record_calls_host.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_record_calls_host_binary_compiles(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout


def leave_one_haplotype_out_of_every_seventh_record(vcf):
    """the first panel haplotype of every seventh record becomes `.`: the index builder gives a missing haplotype an allele of
    its own, `N`, whose sequence is undefined"""
    lines, n, k = [], 0, 0
    for line in vcf.read_text().splitlines():
        c = line.split("\t")
        if not line.startswith("#"):
            k += 1
            if k % 7 == 0:
                c[9] = "." + c[9][c[9].index("|"):]
                n += 1
        lines.append("\t".join(c))
    vcf.write_text("\n".join(lines) + "\n")
    return n


@pytest.mark.gpu
def test_cohort_record_calls_equal_the_vcf_text(binary, tmp_path):
    # a pangenome of 150 kb, 300 records, 8 panel samples (16 paths), indexed by the host index builder; two samples' reads
    q = tmp_path / "q"
    sim = [sys.executable, str(build.ROOT / "tools" / "simulate_pangenome.py")]
    subprocess.run(sim + ["panel", "150000", "300", "8", "11", str(q)], check=True, stdout=subprocess.DEVNULL, timeout=300)
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
    assert r.stdout.count("ok  ") == 1
