"""The sampled-panel VCF of a sampled cohort from the device (C++ host interface: pangenie::sample_cohort_panel_text and
sample_cohort_panel_lines over pg_sampler_cohort_new without sampled_paths, pg_job_record_plan_strided, pg_job_panel_text,
pg_job_panel_line_prefix_strided with Graph::sampled_panel_fixed_columns_slotted, pg_job_panel_lines and the packed fetches;
DESIGN.md 4e-10): tests/cpp/test_panel_host.cpp, compiled the way the host tests are, compares every sample's lines with
Graph::sampled_panel_records over the SampledPanels the host makes of genotype_cohort_sampled(..., &sampled), line for line, and
reads the file written by Graph::write_sampled_panel(RecordLines) back — on the reference's region fixture (its counts as two
samples), then with a REF of undefined sequence: the host route inside the drivers.  Without a device: the refusals."""
import shutil
import subprocess

import pytest

from pangenie_amd import build

GOLDEN = build.ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    build.build_host()
    cxx = shutil.which("g++") or "g++"
    exe = tmp_path_factory.mktemp("cpp") / "test_panel_host"
    host, csrc = build.ROOT / "pangenie_amd" / "host", build.ROOT / "pangenie_amd" / "csrc"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", str(build.ROOT / "tests" / "cpp" / "test_panel_host.cpp"), "-o", str(exe),
           f"-L{host}", "-lpangenie_host", f"-L{csrc}", "-lpangenie_hmm", "-lz", "-lpthread", "-ldl", f"-Wl,-rpath,{host}:{csrc}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def passed(r, n_ok):
    print(r.stdout[-4000:])
    assert r.returncode == 0 and " 0 failed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.count("ok  ") == n_ok


def test_the_refusals_need_no_device(binary, tmp_path):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
    passed(subprocess.run([binary, "cpu"], capture_output=True, text=True, timeout=120, cwd=tmp_path), 1)


@pytest.mark.gpu
def test_the_region_fixture_its_counts_as_two_samples_and_the_host_route(binary, tmp_path):
    passed(subprocess.run([binary, "counted", str(GOLDEN / "region_UniqueKmersList.cereal"), str(GOLDEN / "index_chr1_Graph.cereal"), "1", "160", "80", "15"],
                          capture_output=True, text=True, timeout=300, cwd=tmp_path), 2)
