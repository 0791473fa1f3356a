"""What the folded block-match metric (weight_mfma, vp8hip_dev.h: the matrix instruction delivers the row butterfly of rows 0 and 2 of
the column pass, so one of the two packed row pairs behind it needs none) costs the two search kernels, counted in the gfx950 code hipcc
emits (no GPU needed).  Both kernels are bound by vector-instruction issue: the count is the cost.  Method and flags:
test_search2_instruction_budget.py, whose loop_valu() is used here.

                                                                              parent    this build
    k_search2_b   reference loop                                     475       443
                           once per group of eight blocks                     53        70     (the producer of the C input: 16 ints per
                                                                                               4x4 block in the new order, half a block per lane)
                           per (group, reference) at three references         492.7     466.3
    k_search1_plr_b        the sub-block loop (its five metric MFMAs)         407       367
                           the reference loop around it                       550       510

Eight instructions per call of the metric, as the instruction stream was planned.  The ceilings are the plan's, not this build's counts."""
import os
import shutil
import subprocess

import pytest

from test_search2_instruction_budget import CSRC, REFS, ROOT, loop_valu

S2_REF_LOOP_MAX = 445
S2_PER_GROUP_MAX = 80
S2_PER_GROUP_REF_MAX = 470
S1_MFMA_LOOP_MAX = 370
S1_REF_LOOP_MAX = 515


def _asm(src, tmp_path):
    out = tmp_path / (src + ".s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", str(out), "-w"], check=True, timeout=600)
    return out.read_text()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_quarter_pel_search_issues_the_folded_metrics_count(tmp_path):
    ref_loop, group_loop, mfma = loop_valu(_asm("kernels_s2.hip", tmp_path), "k_search2_bE")
    per_group = group_loop - ref_loop
    per_group_ref = ref_loop + per_group / REFS
    print(f"k_search2_b: reference loop {ref_loop} (parent 475), once per group {per_group} (parent 53), per (group, reference) at "
          f"{REFS} references {per_group_ref:.1f} (parent 492.7)")
    assert mfma == 8, mfma
    assert ref_loop <= S2_REF_LOOP_MAX, (ref_loop, S2_REF_LOOP_MAX)
    assert 0 < per_group <= S2_PER_GROUP_MAX, (per_group, S2_PER_GROUP_MAX)
    assert per_group_ref <= S2_PER_GROUP_REF_MAX, (per_group_ref, S2_PER_GROUP_REF_MAX)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_whole_pel_search_issues_the_folded_metrics_count(tmp_path):
    mfma_loop, ref_loop, mfma = loop_valu(_asm("kernels_me.hip", tmp_path), "k_search1_plr_b")
    print(f"k_search1_plr_b: the loop holding its {mfma} metric MFMAs {mfma_loop} (parent 407), the loop around it {ref_loop} (parent 550)")
    assert mfma == 5, mfma
    assert mfma_loop <= S1_MFMA_LOOP_MAX, (mfma_loop, S1_MFMA_LOOP_MAX)
    assert mfma_loop < ref_loop <= S1_REF_LOOP_MAX, (ref_loop, S1_REF_LOOP_MAX)
