"""Compile-time guard for the kernels that share the lean column step (pg_kernels.hip: lean_states), from the code object's
metadata alone (CPU: hipcc cross-compiles gfx950 without a GPU), in the manner of tests/test_kernel_resources.py.

A row pair of the step now holds both states' sums at once.  The lone-chain sweeps k_sweep_lean<1>, <3>, <4> and k_refill_lean
had no scratch before and must have none.  The triangle kernels and k_sweep_lean2 stand at 256 VGPRs with a few bytes of scratch
a lane (the triangle factors and units per row pair; profiles/r18_lean_upkeep.txt: 156, 12 and 36 bytes) and run two workgroups a
CU: they keep two waves a SIMD, and their scratch stays within a few registers of what it was."""
import re
import subprocess
from pathlib import Path

import pytest

from pangenie_amd import build

SRC = Path(build.__file__).resolve().parent / "csrc" / "pg_kernels.hip"
NO_SCRATCH = ("_Z12k_sweep_leanILi1ELi16ELb0EEvPK9DevContigj", "_Z12k_sweep_leanILi3ELi16ELb0EEvPK9DevContigj",
              "_Z12k_sweep_leanILi4ELi16ELb0EEvPK9DevContigj", "_Z13k_refill_leanILi16EEvPK9DevContigjjjj")
# kernel -> bytes of scratch a lane it may have: the commit before had 156, 12 and 36; a pair now holds both states' sums at once
# (two registers more where there are none to spare: tri<3> has 24)
TWO_WAVES = {"_Z16k_sweep_lean_triILi1ELi16EEvPK9DevContigj": 156, "_Z16k_sweep_lean_triILi3ELi16EEvPK9DevContigj": 24,
             "_Z13k_sweep_lean2ILi16EEvPK9DevContig": 36}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "pg_kernels.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
           "-Wno-unused-value", "-Wno-unused-result", "-mllvm", "-amdgpu-mfma-vgpr-form", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def metadata_of(text, name):
    i = text.index(".name:           " + name + "\n")
    j = text.rfind("\n  - .", 0, i)
    k = text.find("\n  - .", i)
    return text[j:k if k > 0 else len(text)]


def field(meta, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def body_of(text, name):
    i = text.index(name + ":")
    return text[i:text.index(".Lfunc_end", i)]


@pytest.mark.parametrize("name", NO_SCRATCH)
def test_lone_chain_kernels_have_no_scratch(asm, name):
    meta = metadata_of(asm, name)
    print(name, "vgpr", field(meta, "vgpr_count"), "sgpr", field(meta, "sgpr_count"), "lds", field(meta, "group_segment_fixed_size"))
    assert field(meta, "private_segment_fixed_size") == 0, meta[:600]
    assert "scratch_" not in body_of(asm, name)
    assert field(meta, "agpr_count") == 0
    assert field(meta, "vgpr_count") <= 256        # (one workgroup of four waves a chain: occupancy is not what bounds a lone chain)
    assert 2 * field(meta, "group_segment_fixed_size") <= 160 * 1024   # a refill segment runs beside a sweep on one CU


@pytest.mark.parametrize("name", sorted(TWO_WAVES))
def test_triangle_kernels_keep_two_waves_a_simd(asm, name):
    meta = metadata_of(asm, name)
    print(name, "vgpr", field(meta, "vgpr_count"), "scratch", field(meta, "private_segment_fixed_size"))
    assert field(meta, "vgpr_count") + field(meta, "agpr_count") <= 256      # 512 registers a SIMD lane: two waves
    assert 2 * field(meta, "group_segment_fixed_size") <= 160 * 1024         # two workgroups a CU
    assert field(meta, "private_segment_fixed_size") <= TWO_WAVES[name], (name, field(meta, "private_segment_fixed_size"))


def test_the_state_block_of_the_store_free_step_has_no_pad(asm):
    """between the first state's DPP statement and the parked partial sum of a store-free step there is no s_nop: every block of
    the sparse phase-1 sweep that holds all sixteen DPP statements and no global store is such a step's"""
    body = body_of(asm, NO_SCRATCH[0])
    blocks = re.split(r"^\.LBB\d+_\d+:", body, flags=re.M)
    steps = [b for b in blocks if len(re.findall(r"v_fmac_f64_dpp", b)) == 16 and "global_store" not in b]
    assert len(steps) >= 4, len(steps)    # both roles, two steps of the loop body each
    for b in steps:
        first = b.index("v_fmac_f64_dpp")
        last = b.find("ds_write", first)     # (the backward role's block ends at the zero test behind the states, in front of the write)
        last = last if last > 0 else len(b)
        assert not re.search(r"\bs_nop\b", b[first:last].replace("s_nop 1\n\t;;#ASMEND", "")), b[first:last]
