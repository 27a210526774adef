"""Compile-time guard for the kernels of pg_combine_records.hip (CPU: hipcc cross-compiles gfx950 without a GPU), read from the
kernels' metadata alone, in the manner of tests/test_record_calls_kernel_resources.py: no kernel has a private segment
(scratch), none spills a register, the lane-per-record kernels hold at most 64 VGPRs (eight waves a SIMD) and the
wave-per-record kernels at most 128.

The VGPR counts are pinned at what the compiler gives today — k_crcalls 52, k_crgl 64, k_crcalls_wide 50, k_crgl_wide 64,
k_crplan_ids 8.  k_crgl sits AT its bound: its store and its vcf_index functor keep the block's base pointers (scalar
registers) and a 32-bit index per lane instead of a pointer per lane, which is what brought it from 66 to 64.  The
wave-per-record kernels keep a record's slot map in LDS: 256 two-byte entries."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_combine_records.hip"
# stem -> (pinned VGPRs, bound, LDS bytes)
KERNELS = {"9k_crcalls": (52, 64, 0), "6k_crgl": (64, 64, 0), "14k_crcalls_wide": (50, 128, 512), "11k_crgl_wide": (64, 128, 512),
           "12k_crplan_ids": (8, 64, 0)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_combine_records.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def metadata_of(text, stem):
    names = sorted(set(re.findall(r"^\s+\.name:\s+(_Z\w*%sE\w*)$" % stem, text, re.M)))
    assert len(names) == 1, (stem, names)
    i = text.index(".name:           " + names[0])
    j = text.rfind("  - .", 0, i)
    k = text.find("\n  - .", i)
    return text[j:k if k > 0 else len(text)]


def field(meta, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, meta).group(1))


def test_the_unit_is_part_of_the_library_and_holds_these_kernels_and_no_other(asm):
    assert SRC in build.HIP_SOURCES
    assert len(re.findall(r"^\s+\.name:\s+_Z\w+$", asm, re.M)) == len(KERNELS)


@pytest.mark.parametrize("stem", sorted(KERNELS))
def test_no_scratch_no_spills_and_the_pinned_registers(asm, stem):
    pinned, bound, lds = KERNELS[stem]
    meta = metadata_of(asm, stem)
    assert field(meta, "private_segment_fixed_size") == 0, meta[:600]
    assert field(meta, "vgpr_spill_count") == 0 and field(meta, "sgpr_spill_count") == 0, meta[:600]
    assert field(meta, "group_segment_fixed_size") == lds, meta[:600]
    vgprs = field(meta, "vgpr_count")
    assert vgprs <= pinned, (stem, vgprs)
    assert pinned <= bound
