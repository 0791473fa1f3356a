"""What the batched whole-pel search (k_search1_plr_b) issues per (block, reference) with the row-order operand and the filled lane map, counted
in the gfx950 code hipcc emits (no GPU needed).  The kernel is bound by vector-instruction issue: the count is the cost.  Method and flags:
test_search2_instruction_budget.py, whose loop_valu() is used here.

  * Row-order operand (s1_subblock_pre): a candidate's B operand is four bytes of each reference row as loaded -- twelve v_alignbyte per sub-block
    where two 4x4 byte transposes and eight register copies stood (24).  The sub-block loop, which holds the five metric MFMAs: 367 -> 351.
  * Filled map (csrc/s1_fill_layout.h): 51 blocks in a workgroup's 256 lanes = 12.75 blocks per wave instead of 12, and the minimum over a block's
    lanes through LDS instead of three shuffle steps.

    dynamic VALU per (block, reference) = ((reference loop - sub-block loop) + 4 x sub-block loop) / blocks per wave
        parent      (143 + 4 x 367) / 12     = 134.3
        this build  (150 + 4 x 351) / 12.75  = 121.9
The ceilings are the plan's (sub-block loop 353; 124 per block and reference = the plan's 121 with 2 % for the barrier and the LDS minimum), not
this build's counts."""
import os
import re
import shutil
import subprocess

import pytest

from test_search2_instruction_budget import CSRC, ROOT, loop_valu

SUBBLOCK_LOOP_MAX = 353
PER_BLOCK_REF_MAX = 124
BLOCKS_PER_WAVE = 51 / 4
LDS_MAX = 16384


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    out = tmp_path_factory.mktemp("s1fill") / "kernels_me.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "kernels_me.hip"), "-o", str(out), "-w"], check=True, timeout=600)
    return out.read_text()


def test_the_filled_search_issues_the_planned_count_per_block_and_reference(asm):
    sub_loop, ref_loop, mfma = loop_valu(asm, "k_search1_plr_b")
    per = ((ref_loop - sub_loop) + 4 * sub_loop) / BLOCKS_PER_WAVE
    print(f"k_search1_plr_b: sub-block loop {sub_loop} (parent 367), reference loop {ref_loop} (parent 510), {mfma} MFMAs, "
          f"per (block, reference) {per:.1f} (parent 134.3)")
    assert mfma == 5, mfma
    assert sub_loop <= SUBBLOCK_LOOP_MAX, (sub_loop, SUBBLOCK_LOOP_MAX)
    assert ref_loop > sub_loop, "no sub-block loop inside the reference loop"
    assert per <= PER_BLOCK_REF_MAX, (per, PER_BLOCK_REF_MAX)


def test_the_filled_searchs_lds_fits_sixteen_kib(asm):
    m = re.search(r"\.amdhsa_kernel _ZN3vp815k_search1_plr_b\w*\n(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert m, "k_search1_plr_b's kernel descriptor not found"
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(1)).group(1))
    print(f"k_search1_plr_b: {lds} bytes of LDS")
    assert 51 * 68 * 4 <= lds <= LDS_MAX, lds
