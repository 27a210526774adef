"""Compile-time guard for the kernels of the path-subset flow in pg_combine.hip (CPU: hipcc cross-compiles gfx950 without a
GPU), in the manner of tests/test_calls_kernel_resources.py: no kernel touches scratch or holds an atomic instruction, a
combined bin leaves as ONE 16-byte vector store and a call as ONE 8-byte one.

The VGPR counts are pinned at what the compiler gives today — k_combine 31, k_combine_wide 44, k_ccalls 36, k_ccalls_wide 37,
k_combine_check 7 — every one of them at most 64, i.e. eight waves a SIMD, the most the hardware holds: occupancy is not what
bounds these kernels.  The pins leave no room: a kernel that grows is looked at."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_combine.hip"
VGPRS = {"9k_combine": 31, "14k_combine_wide": 44, "8k_ccalls": 36, "13k_ccalls_wide": 37, "15k_combine_check": 7}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_combine.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def kernel(text, stem):
    names = sorted(set(re.findall(r"^(_Z\w*%sE\w*):" % stem, text, re.M)))
    assert len(names) == 1, names
    return names[0]


def body_of(text, name):
    i = text.index(name + ":")
    return text[i:text.index(".Lfunc_end", i)]


def metadata_of(text, name):
    i = text.index(".name:           " + name)
    j = text.rfind("  - .", 0, i)
    k = text.find("\n  - .", i)
    return text[j:k if k > 0 else len(text)]


def test_the_unit_holds_these_kernels_and_no_other(asm):
    assert len(re.findall(r"^\s+\.name:\s+_Z\w+$", asm, re.M)) == len(VGPRS)


@pytest.mark.parametrize("stem", sorted(VGPRS))
def test_no_scratch_no_atomics_and_the_pinned_registers(asm, stem):
    name = kernel(asm, stem)
    body, meta = body_of(asm, name), metadata_of(asm, name)
    assert re.search(r"\.symbol:\s+%s\.kd" % re.escape(name), meta), meta[:400]
    assert "scratch_" not in body
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert not re.search(r"atomic|cmpswap", body)
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    assert vgprs <= VGPRS[stem], (stem, vgprs)
    assert vgprs <= 64      # eight waves a SIMD


@pytest.mark.parametrize("stem", ["9k_combine", "14k_combine_wide"])
def test_a_combined_bin_leaves_as_one_16_byte_store(asm, stem):
    body = body_of(asm, kernel(asm, stem))
    assert re.search(r"\b(global|flat)_store_dwordx4\b", body)
    assert not re.search(r"\b(global|flat)_store_(byte|short|dword|dwordx2|dwordx3)\b", body)   # nothing leaves but whole bins


@pytest.mark.parametrize("stem", ["8k_ccalls", "13k_ccalls_wide"])
def test_a_call_leaves_as_one_8_byte_store_and_needs_no_lds(asm, stem):
    name = kernel(asm, stem)
    body, meta = body_of(asm, name), metadata_of(asm, name)
    assert re.search(r"\b(global|flat)_store_dwordx2\b", body)
    assert not re.search(r"\b(global|flat)_store_(byte|short|dword|dwordx3|dwordx4)\b", body)   # nothing leaves but whole records
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", meta), meta[:400]
