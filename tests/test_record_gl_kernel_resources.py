"""Compile-time guard for the three kernels of the GL column in pg_calls.hip (CPU: hipcc cross-compiles gfx950 without a GPU).
Only the kernels' METADATA is read: none touches scratch or spills — the narrow kernel walks the bubble's keys once per
genotype pair precisely so that no array indexed at run time exists — and each stays within 128 VGPRs, four waves a SIMD of
the 512-register file (found: 70 for k_rgl, 70 for k_rgl_wide, 25 for k_gl_values)."""
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


@pytest.mark.parametrize("stem,lds", [("5k_rgl", 0), ("10k_rgl_wide", 512), ("11k_gl_values", 0)])
def test_no_scratch_no_spills_and_four_waves_a_simd(asm, stem, lds):
    meta = metadata_of(asm, stem)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta[:400]
    assert re.search(r"\.sgpr_spill_count:\s+0\b", meta), meta[:400]
    assert re.search(r"\.group_segment_fixed_size:\s+%d\b" % lds, meta), meta[:400]   # the wide kernel: one u16 per allele slot
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 128
