"""The phasing VCF with its GT:KC column formed on the device (C++ host interface: pangenie::phase_cohort_record_text and
phase_cohort_record_lines over pg_job_phased_text, pg_job_phased_line_prefix, pg_job_phased_lines and their packed fetches;
Graph::phasing_fixed_columns, phasing_header(samples), phasing_records(RecordText), write_phasing(RecordLines)):
tests/cpp/test_phase_host.cpp, compiled the way the host tests are, compares the drivers line for line with
Graph::phasing_records over the results of an HMM that runs the phasing alone — on the reference's region fixture over 30 of
its 215 paths, one sample and the same counts as two, with and without ignore_imputed, once more with every ALT of undefined
sequence (`.` on the device route) and once with a REF of undefined sequence, which the drivers send down the host route.  The
demo's phasing run through the device route pins what tests/golden/demo/test_phasing.vcf pins of the host route
(tests/test_demo.py: check_phasing; the file's UK and KC are an older release's, so it cannot be met text for text).  Without a device: the fixed
columns against whole lines, the multi-sample header, the file, the refusals."""
import shutil
import subprocess

import pytest

from pangenie_amd import build
from tests.test_demo import check_phasing

GOLDEN = build.ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_phase_host"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_phase_host.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def passed(r, n_ok):
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == n_ok


def test_the_fixed_columns_the_header_the_file_and_the_refusals(binary, tmp_path):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
    passed(subprocess.run([binary, "cpu", str(GOLDEN / "index_chr1_Graph.cereal")], capture_output=True, text=True, timeout=120, cwd=tmp_path), 5)


@pytest.mark.gpu
def test_the_region_fixture_one_sample_two_and_the_host_route(binary, tmp_path):
    passed(subprocess.run([binary, "counted", str(GOLDEN / "region_UniqueKmersList.cereal"), str(GOLDEN / "index_chr1_Graph.cereal"), "1", "160", "80", "30"],
                          capture_output=True, text=True, timeout=300, cwd=tmp_path), 4)


@pytest.mark.gpu
def test_the_demos_phasing_run_through_the_device_route(binary, tmp_path):
    prefix = tmp_path / "preprocessing"
    r = subprocess.run([str(build.HOST_TEST), "demo-counts", str(GOLDEN / "demo"), str(prefix), "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    peak = int(r.stdout.strip().split("=")[1])
    out = tmp_path / "test_phasing.vcf"
    r = subprocess.run([binary, "vcf", str(prefix) + "_counted_UniqueKmersMap.cereal", str(prefix) + "_chr1_Graph.cereal", str(peak // 4), str(peak * 4),
                        str(2 * peak), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    check_phasing(out.read_text())
