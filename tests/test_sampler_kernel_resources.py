"""Compile-time guard for the sampled-cohort kernels of pg_sampler.hip (CPU: hipcc cross-compiles gfx950 without a GPU), shaped
like tests/test_kernel_resources.py: the emission cost kernel (a loop over a variant's alleles and their k-mer bits) and the
per-chain slot copy touch no scratch at all — not in their large blocks, not anywhere — and keep a small register footprint
(they run over thousands of chains in one launch)."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_sampler.hip"

KERNELS = ("_ZN12_GLOBAL__N_18ks_ecostEPKNS_7CostDevEPKt", "_ZN12_GLOBAL__N_112ks_slot_copyEPKNS_7CostDevE")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_sampler.s"
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


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(asm, kernel):
    body = body_of(asm, kernel)
    assert "scratch_" not in body, kernel
    meta = metadata_of(asm, kernel)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    assert vgprs <= 32, vgprs
