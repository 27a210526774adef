"""Compile-time guard for the kernels of the record text in pg_record_text.hip (CPU: hipcc cross-compiles gfx950 without a GPU).
Only the kernels' METADATA is read: none touches scratch — every character goes through a sink, no array is indexed at run
time — none spills, and each stays within the LDS it declares: k_rtext_emit its 32 KB stage and the block's 257 offsets, 256
flags and the window (four workgroups share a CU's 160 KB), k_rtext_emit_wide its 4 KB stage, the scans a word per wave.  All
stay within 64 VGPRs, the step at which eight waves share a SIMD."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_record_text.hip"
STAGE = 32768


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_record_text.s"
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


def test_the_unit_is_part_of_the_library():
    assert SRC in build.HIP_SOURCES
    assert "#define RT_STAGE %du" % STAGE in SRC.read_text()


@pytest.mark.parametrize("stem,lds_min,lds_max", [
    ("11k_rtext_len", 16, 16), ("16k_rtext_len_wide", 0, 0), ("12k_rtext_sums", 32, 32),
    ("12k_rtext_emit", STAGE, STAGE + 257 * 4 + 256 + 8 + 512), ("17k_rtext_emit_wide", 4096, 4096)])
def test_no_scratch_no_spills_and_the_declared_lds(asm, stem, lds_min, lds_max):
    meta = metadata_of(asm, stem)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta[:400]
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta).group(1))
    assert lds_min <= lds <= lds_max, lds
    assert lds * 4 <= 160 * 1024
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64
