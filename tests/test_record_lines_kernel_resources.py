"""Compile-time guard for the kernels of the record lines in pg_record_lines.hip (CPU: hipcc cross-compiles gfx950 without a GPU).
The unit holds five kernels: k_rlines_sums, and k_rlines_len and k_rlines_emit once for plain prefixes (SLOT = false) and once
for slotted ones (SLOT = true).  Only the kernels' METADATA is read: none touches scratch (the number piece is formed in a
register, not in a local array), none spills, and each stays within the LDS it declares: k_rlines_emit its 8 KB stage and the
65 line starts of its wave, the scans a word per wave — far more than two workgroups share a CU's 160 KB.  All stay within 64
VGPRs, the step at which eight waves share a SIMD, and no instantiation takes more VGPRs than the kernel of its role took while
plain and slotted prefixes had a unit each: the plain path pays nothing for sharing its source."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

CSRC = Path(build.__file__).resolve().parent / "csrc"
SRC = CSRC / "pg_record_lines.hip"
STAGE = 8192
EMIT_LDS = (STAGE, STAGE + 65 * 4 + 64)
# kernel -> the stem of its mangled name (the template argument Lb0E / Lb1E is SLOT), its LDS window, and the VGPRs of the
# separate kernel of that role at the commit before the units were joined (k_rlines_sums did not change: the 64 of all)
KERNELS = {
    "k_rlines_len<false>": ("12k_rlines_lenILb0EE", (16, 16), 13),
    "k_rlines_len<true>": ("12k_rlines_lenILb1EE", (16, 16), 13),
    "k_rlines_sums": ("13k_rlines_sumsE", (32, 32), 64),
    "k_rlines_emit<false>": ("13k_rlines_emitILb0EE", EMIT_LDS, 42),
    "k_rlines_emit<true>": ("13k_rlines_emitILb1EE", EMIT_LDS, 46),
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_record_lines.s"
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
    assert SRC in build.HIP_SOURCES and CSRC / "pg_shim_lines.cpp" in build.HIP_SOURCES
    assert "#define RL_STAGE %du" % STAGE in SRC.read_text()
    # the wave scan, the sums scan and the flush exist once, in the header both units include
    shared = (CSRC / "pg_text_scan.h").read_text()
    for unit in (SRC, CSRC / "pg_record_text.hip"):
        text = unit.read_text()
        assert '#include "pg_text_scan.h"' in text
        for helper in ("uint32_t wave_incl_scan(", "void rtext_flush(", "void block_sums_scan("):
            assert helper in shared and helper not in text, (unit.name, helper)


def test_the_slotted_kernels_use_the_shared_helpers_and_no_copy():
    # what the slotted unit's test asked of its file, asked of the one unit that now holds the slotted kernels
    assert SRC in build.HIP_SOURCES
    text = SRC.read_text()
    assert "template <bool SLOT>" in text and "#define RL_STAGE %du" % STAGE in text
    shared = (CSRC / "pg_text_scan.h").read_text()
    assert '#include "pg_text_scan.h"' in text
    for helper in ("uint32_t wave_incl_scan(", "uint32_t block_excl_scan(", "void block_sums_scan(", "void rtext_flush("):
        assert helper in shared and helper not in text, helper
        assert helper.split()[-1][:-1] in text, helper   # ... and are used here


def test_slotted_prefixes_have_no_unit_of_their_own():
    gone = CSRC / "pg_record_lines_slot.hip"
    assert not gone.exists()
    assert gone not in build.HIP_SOURCES and all(p.name != gone.name for p in build.HIP_SOURCES)


def test_these_are_all_the_kernels_of_the_unit(asm):
    # every kernel's name begins with one of the five stems and no two share one: a sixth kernel, or a third instantiation, fails
    names = kernel_names(asm)
    stems = sorted(stem for stem, _, _ in KERNELS.values())
    assert len(names) == len(stems) and all(n.startswith(s) for n, s in zip(names, stems)), names


def test_the_slotted_kernels_are_one_len_one_emit_and_the_shared_sums(asm):
    # the slotted unit had exactly k_rlslot_emit, k_rlslot_len and k_rlslot_sums: now the SLOT = true instantiations and the one sums
    names = kernel_names(asm)
    slotted = [n for n in names if "ILb1E" in n]
    assert len(slotted) == 2 and slotted[0].startswith("12k_rlines_lenILb1EE") and slotted[1].startswith("13k_rlines_emitILb1EE"), names
    assert [n for n in names if "ILb" not in n] == [n for n in names if n.startswith("13k_rlines_sumsE")] and sum("sums" in n for n in names) == 1, names


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spills_and_the_declared_lds(asm, kernel):
    stem, (lds_min, lds_max), vgprs_before = KERNELS[kernel]
    meta = metadata_of(asm, stem)
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), meta[:400]
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), meta[:400]
    assert re.search(r"\.sgpr_spill_count:\s+0\b", meta), meta[:400]
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta).group(1))
    assert lds_min <= lds <= lds_max, lds
    assert lds * 2 <= 160 * 1024   # at least two workgroups a CU
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    assert vgprs <= 64 and vgprs <= vgprs_before, vgprs
