"""Compile-time guard for the kernels of the count plan in pg_kmers.hip (CPU: hipcc cross-compiles gfx950 without a GPU), in
the manner of tests/test_kmers_kernel_resources.py: neither kernel touches scratch, and the fill kernel — a gather and
plain stores — holds no atomic instruction of any kind and no LDS."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_kmers.hip"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_kmers.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
           "-Wno-unused-value", "-Wno-unused-result", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def kernels(text, stem):
    """mangled names of every instantiation of a kernel template (32- and 64-bit slot indices)"""
    names = sorted(set(re.findall(r"^(_Z\w*%s\w*):" % stem, text, re.M)))
    assert len(names) == 2, names
    return names


def body_of(text, name):
    i = text.index(name + ":")
    return text[i:text.index(".Lfunc_end", i)]


def metadata_of(text, name):
    i = text.index(".name:           " + name)
    j = text.rfind("  - .", 0, i)
    k = text.find("\n  - .", i)
    return text[j:k if k > 0 else len(text)]


@pytest.mark.parametrize("stem", ["kk_plan_fill", "kk_plan_resolve"])
def test_no_scratch(asm, stem):
    for kernel in kernels(asm, stem):
        assert "scratch_" not in body_of(asm, kernel), kernel
        meta = metadata_of(asm, kernel)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]


def wide_and_narrow(text, stem):
    """(the instantiation for uint64_t slot indices, the one for uint32_t): `m` and `j` in the mangled template argument"""
    names = kernels(text, stem)
    wide = [n for n in names if re.search(r"%sImE" % stem, n)]
    narrow = [n for n in names if re.search(r"%sIjE" % stem, n)]
    assert len(wide) == 1 and len(narrow) == 1, names
    return wide[0], narrow[0]


@pytest.mark.parametrize("stem", ["kk_plan_fill", "kk_plan_resolve"])
def test_the_wide_instantiations_are_in_the_code_object_and_meet_the_same_bounds(asm, stem):
    """the kernels of a table of 2^32 slots or more (PG_COUNT_PLAN=wide runs them on small tables: tests/test_counts_wide_gpu.py)"""
    wide, narrow = wide_and_narrow(asm, stem)
    for kernel in (wide, narrow):
        meta = metadata_of(asm, kernel)
        assert re.search(r"\.symbol:\s+%s\.kd" % re.escape(kernel), meta), meta[:400]   # a kernel of the code object, not a name in passing
        assert "scratch_" not in body_of(asm, kernel), kernel
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    if stem == "kk_plan_fill":
        body, meta = body_of(asm, wide), metadata_of(asm, wide)
        assert not re.search(r"atomic|cmpswap", body)
        assert re.search(r"\b(global|flat)_store_short\b", body) and "global_load_dwordx2" in body
        assert re.search(r"\.group_segment_fixed_size:\s+0\b", meta), meta[:400]
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64
    else:
        # the slot index leaves as 8 bytes in the wide kernel, as 4 in the narrow one
        assert re.search(r"\bglobal_store_dwordx2\b", body_of(asm, wide)) and not re.search(r"\bglobal_store_dwordx2\b", body_of(asm, narrow))


def test_fill_kernel_only_gathers_and_stores(asm):
    for kernel in kernels(asm, "kk_plan_fill"):
        body = body_of(asm, kernel)
        assert not re.search(r"atomic|cmpswap", body), kernel
        # (the output pointers come out of the descriptor table, so the 2-byte stores are flat ones: plain vector stores)
        assert re.search(r"\b(global|flat)_store_short\b", body) and "global_load_dwordx2" in body
        meta = metadata_of(asm, kernel)
        assert re.search(r"\.group_segment_fixed_size:\s+0\b", meta), meta[:400]
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64   # eight waves a SIMD: the kernel lives on loads in flight
