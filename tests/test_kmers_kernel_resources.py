"""Compile-time guard for the kernels of pg_kmers.hip (CPU: hipcc cross-compiles gfx950 without a GPU), shaped like
tests/test_sampler_kernel_resources.py: the counting and the lookup kernel touch no scratch, and the counting kernel's
increment is ONE native 64-bit atomic add — an increment that became a compare-and-swap loop is a regression."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_kmers.hip"

COUNT = "_ZN12_GLOBAL__N_18kk_countEPKcmjPNS_4SlotEmPy"
LOOKUP = "_ZN12_GLOBAL__N_19kk_lookupEPKymPKNS_4SlotEmPy"
REGISTER = "_ZN12_GLOBAL__N_111kk_registerEPKcmjPymS2_"


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


def body_of(text, name):
    i = text.index(name + ":")
    return text[i:text.index(".Lfunc_end", i)]


def metadata_of(text, name):
    i = text.index(".name:           " + name)
    j = text.rfind("  - .", 0, i)   # the metadata entry of this kernel starts before its name
    k = text.find("\n  - .", i)
    return text[j:k if k > 0 else len(text)]


@pytest.mark.parametrize("kernel", [COUNT, LOOKUP, REGISTER])
def test_no_scratch(asm, kernel):
    body = body_of(asm, kernel)
    assert "scratch_" not in body, kernel
    meta = metadata_of(asm, kernel)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]


def test_counting_kernel_increments_with_one_native_atomic(asm):
    body = body_of(asm, COUNT)
    assert "global_atomic_add_x2" in body
    assert "global_atomic_cmpswap" not in body
    # no-return form: a returning atomic (sc0) would make every lane wait for its own increment
    adds = re.findall(r"global_atomic_add_x2[^\n]*", body)
    assert adds and not any(" sc0" in a for a in adds), adds[:3]


def test_counting_kernel_has_sixteen_probes_in_flight(asm):
    """the first probes of a lane's 16 windows are issued back to back, before anything waits for the first of them"""
    body = body_of(asm, COUNT)
    runs, run = [], 0
    for line in body.splitlines():
        line = line.strip()
        if line.startswith("global_load_dwordx2"):
            run += 1
        elif line.startswith("s_waitcnt") and "vmcnt" in line:
            runs.append(run)
            run = 0
    assert max(runs + [run]) >= 16, runs


def test_counting_kernel_keeps_four_waves_a_simd(asm):
    meta = metadata_of(asm, COUNT)
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 128
