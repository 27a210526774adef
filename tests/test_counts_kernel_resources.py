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


def test_fill_kernel_only_gathers_and_stores(asm):
    for kernel in kernels(asm, "kk_plan_fill"):
        body = body_of(asm, kernel)
        assert not re.search(r"atomic|cmpswap", body), kernel
        # (the output pointers come out of the descriptor table, so the 2-byte stores are flat ones: plain vector stores)
        assert re.search(r"\b(global|flat)_store_short\b", body) and "global_load_dwordx2" in body
        meta = metadata_of(asm, kernel)
        assert re.search(r"\.group_segment_fixed_size:\s+0\b", meta), meta[:400]
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64   # eight waves a SIMD: the kernel lives on loads in flight
