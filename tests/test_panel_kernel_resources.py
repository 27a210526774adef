"""Compile-time guard for the kernels of the sampled panel's columns in pg_panel_text.hip (CPU: hipcc cross-compiles gfx950
without a GPU).  The unit holds three kernels: k_ptpanel_len, k_ptpanel_sums and k_ptpanel_emit.  Only the kernels' METADATA is
read: none touches scratch (the digits go through a sink, no local array is indexed), none spills, all stay within 64 VGPRs —
the step at which eight waves share a SIMD — and each stays within the LDS it declares, far below 64 KB: k_ptpanel_emit its stage
of 256 cells of 4 bytes and the 16 of the residue plus a word per wave for its own scan, the two scans a word per wave.  The
scans and the flush are the shared ones of pg_text_scan.h, used and not copied."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

CSRC = Path(build.__file__).resolve().parent / "csrc"
SRC = CSRC / "pg_panel_text.hip"
STAGE = 256 * 4 + 16
# kernel -> the stem of its mangled name and its LDS in bytes
KERNELS = {
    "k_ptpanel_len": ("13k_ptpanel_lenE", 16),
    "k_ptpanel_sums": ("14k_ptpanel_sumsE", 32),
    "k_ptpanel_emit": ("14k_ptpanel_emitE", STAGE + 16),
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_panel_text.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def kernel_names(text):
    """The mangled name of every kernel in the metadata, without the prefix of the anonymous namespace."""
    return sorted(set(re.findall(r"^\s+\.name:\s+_ZN\d+_GLOBAL__N_1(\w+)$", text, re.M)))


def metadata_of(text, stem):
    names = [n for n in kernel_names(text) if n.startswith(stem)]
    assert len(names) == 1, names
    i = text.index(".name:           _ZN12_GLOBAL__N_1" + names[0])
    j = text.rfind("  - .", 0, i)
    k = text.find("\n  - .", i)
    return text[j:k if k > 0 else len(text)]


def test_the_unit_is_part_of_the_library_and_shares_its_helpers():
    assert SRC in build.HIP_SOURCES and CSRC / "pg_shim_panel.cpp" in build.HIP_SOURCES
    text = SRC.read_text()
    assert '#include "pg_panel.h"' in text and '#include "pg_text_scan.h"' in text
    assert "#define PP_STAGE (PP_BLOCK * PP_CELL_BYTES + 16u)" in text and "#define PP_CELL_BYTES 4u" in text
    # the wave scan, the block scan, the sums scan and the flush exist once, in the header the units of packed text include
    shared = (CSRC / "pg_text_scan.h").read_text()
    for helper in ("uint32_t wave_incl_scan(", "uint32_t block_excl_scan(", "void block_sums_scan(", "void rtext_flush("):
        assert helper in shared and helper not in text, helper
    for used in ("block_excl_scan(", "block_sums_scan(", "rtext_flush<"):   # (wave_incl_scan: inside block_excl_scan)
        assert used in text, used
    code = text.split("#include", 1)[1]   # (the header comment says there are none)
    assert "atomic" not in code and "asm" not in code
    # the siblings are as they were: none includes the rule of the panel's columns
    for sibling in ("pg_record_text.hip", "pg_record_lines.hip", "pg_phase_text.hip"):
        assert "pg_panel" not in (CSRC / sibling).read_text()


def test_these_are_all_the_kernels_of_the_unit(asm):
    names = kernel_names(asm)
    stems = sorted(stem for stem, _ in KERNELS.values())
    assert len(names) == len(stems) and all(n.startswith(s) for n, s in zip(names, stems)), names


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spills_and_the_declared_lds(asm, kernel):
    stem, lds_declared = KERNELS[kernel]
    meta = metadata_of(asm, stem)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta[:400]
    assert re.search(r"\.sgpr_spill_count:\s+0\b", meta), meta[:400]
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta).group(1))
    assert lds == lds_declared and lds <= 64 * 1024, lds   # its declared stage and no more
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    print(kernel, "vgprs", vgprs, "lds", lds)
    assert vgprs <= 64, vgprs
