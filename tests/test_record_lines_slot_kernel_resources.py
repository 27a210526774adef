"""Compile-time guard for the kernels of the record lines over slotted prefixes in pg_record_lines_slot.hip (CPU: hipcc
cross-compiles gfx950 without a GPU).  Only the kernels' METADATA is read: none touches scratch (the number piece is formed in
a register, not in a local array), none spills, and each stays within the LDS it declares: k_rlslot_emit its 8 KB stage and the
65 line starts of its wave, the scans a word per wave.  All stay within 64 VGPRs, the step at which eight waves share a SIMD."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

CSRC = Path(build.__file__).resolve().parent / "csrc"
SRC = CSRC / "pg_record_lines_slot.hip"
STAGE = 8192


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_record_lines_slot.s"
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


def test_the_unit_is_part_of_the_library_and_shares_the_helpers():
    assert SRC in build.HIP_SOURCES and CSRC / "pg_record_lines.hip" in build.HIP_SOURCES
    text = SRC.read_text()
    assert "#define RLS_STAGE %du" % STAGE in text
    # the wave scan, the block scan, the sums scan and the flush exist once, in the header the three units include
    shared = (CSRC / "pg_text_scan.h").read_text()
    assert '#include "pg_text_scan.h"' in text
    for helper in ("uint32_t wave_incl_scan(", "uint32_t block_excl_scan(", "void block_sums_scan(", "void rtext_flush("):
        assert helper in shared and helper not in text, helper
        assert helper.split()[-1][:-1] in text, helper   # ... and are used here


def test_these_are_all_the_kernels_of_the_unit(asm):
    kernels = sorted(set(re.findall(r"^\s+\.name:\s+_ZN\d+_GLOBAL__N_1\d+(k_\w+?)E\w*$", asm, re.M)))
    assert kernels == ["k_rlslot_emit", "k_rlslot_len", "k_rlslot_sums"], kernels


@pytest.mark.parametrize("stem,lds_min,lds_max", [
    ("12k_rlslot_len", 16, 16), ("13k_rlslot_sums", 32, 32), ("13k_rlslot_emit", STAGE, STAGE + 65 * 4 + 64)])
def test_no_scratch_no_spills_and_the_declared_lds(asm, stem, lds_min, lds_max):
    meta = metadata_of(asm, stem)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta[:400]
    assert re.search(r"\.sgpr_spill_count:\s+0\b", meta), meta[:400]
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta).group(1))
    assert lds_min <= lds <= lds_max, lds
    assert lds * 2 <= 160 * 1024   # at least two workgroups a CU
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64
