"""Compile-time guard for the kernels of the genotype calls in pg_calls.hip (CPU: hipcc cross-compiles gfx950 without a GPU),
in the manner of tests/test_counts_kernel_resources.py: neither kernel touches scratch (the narrow kernel walks a variant's
bins three times precisely so that no array indexed at run time exists), neither holds an atomic instruction or LDS, and a
record leaves as ONE 8-byte vector store."""
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


@pytest.mark.parametrize("stem", ["7k_calls", "12k_calls_wide"])
def test_no_scratch_no_atomics_no_lds_one_store_per_record(asm, stem):
    name = kernel(asm, stem)
    body, meta = body_of(asm, name), metadata_of(asm, name)
    assert re.search(r"\.symbol:\s+%s\.kd" % re.escape(name), meta), meta[:400]
    assert "scratch_" not in body
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert not re.search(r"atomic|cmpswap", body)
    assert re.search(r"\b(global|flat)_store_dwordx2\b", body)
    assert not re.search(r"\b(global|flat)_store_(byte|short|dword)\b", body)   # nothing leaves but whole records
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64      # eight waves a SIMD
