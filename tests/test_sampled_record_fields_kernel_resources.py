"""Compile-time guard for k_rplan_ids, the id check of the record plans in pg_calls.hip (CPU: hipcc cross-compiles gfx950
without a GPU).  Only the kernel's METADATA is read: it touches no scratch, spills nothing, needs no LDS — one lane per record,
a loop over the bubble's allele ids, one 64-bit atomic on a hit — and stays far within 128 VGPRs (found: 8, with 24 SGPRs)."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_calls.hip"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_calls.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def metadata_of(text, stem):
    names = sorted(set(re.findall(r"^\s+\.name:\s+(_Z\w*%sE\w*)$" % stem, text, re.M)))
    assert len(names) == 1, names
    i = text.index(".name:           " + names[0])
    j = text.rfind("  - .", 0, i)
    k = text.find("\n  - .", i)
    return text[j:k if k > 0 else len(text)]


def test_the_id_check_has_no_scratch_no_spills_and_no_lds(asm):
    meta = metadata_of(asm, "11k_rplan_ids")
    print(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(0), re.search(r"\.sgpr_count:\s+(\d+)", meta).group(0))
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta[:400]
    assert re.search(r"\.sgpr_spill_count:\s+0\b", meta), meta[:400]
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 128
