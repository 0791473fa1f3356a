"""Register / scratch budget of the hot kernels, read from the gfx950 code hipcc emits (no GPU needed).

A kernel argument block that is indexed by a per-lane value gets copied to scratch memory without a word from the compiler
(k_mb did, once: 21 -> 38 us per 1080p frame), and a register count past 128 halves k_mb's waves per SIMD; both are
invisible to the parity tests."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vp8oclenc_amd", "csrc")
HOT = {   # file -> {kernel name fragment: max VGPRs}
    "kernels_mb.hip": {"k_mb_pE": 128, "k_mb_p_conformant": 128},     # four waves per SIMD
    "kernels_s2.hip": {"k_search2E": 72, "k_search2_bE": 72, "k_search2_bsE": 72},      # seven waves per SIMD ... (one video: one group of eight blocks per workgroup; batches: two in a loop)
    "kernels_me.hip": {"k_search1": 128, "k_search1_plE": 64, "k_search1_plr_b": 72, "k_search1_coarse": 64, "k_pyramid": 128, "k_pack_b": 64},   # the loop form: eight (a form with 7 % fewer instructions and 75 registers was no faster)
    "kernels_lf4.hip": {"k_loop_filter4E": 128, "k_loop_filter4_bE": 128,
                        "k_loop_filter4_conformantE": 128, "k_loop_filter4_b_conformantE": 128},   # (87 each, as the default pair: the saturated hand-over shares its clamps with the stores)
    # the banded body of lf_banded.h under its two filter policies: what the shared body must not lose
    "kernels_lf3.hip": {"k_loop_filter3_bE": 90, "k_loop_filter3_b_conformantE": 90},
    "kernels_lf_simple.hip": {"k_loop_filter_simpleE": 80, "k_loop_filter_simple_bE": 80},
}
LDS = {"k_search2E": 23296, "k_search2_bE": 23296, "k_search2_bsE": 23296,   # ... and seven workgroups per CU (163 840 / 7)
       "k_loop_filter3_bE": 47424, "k_loop_filter3_b_conformantE": 47424, "k_loop_filter_simpleE": 47384, "k_loop_filter_simple_bE": 47384}
MFMA = {"k_search2E", "k_search2_bE", "k_search2_bsE"}   # an MFMA result must land in VGPRs (no AGPRs)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
@pytest.mark.parametrize("src", sorted(HOT))
def test_hot_kernels_use_no_scratch_and_stay_inside_their_register_budget(src, tmp_path):
    out = tmp_path / "k.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", str(out), "-w"], check=True, timeout=600)
    text = out.read_text()
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:.*\n)*?)\s+\.wavefront_size", text):
        name, body = m.group(1), m.group(2)
        for frag, max_vgprs in HOT[src].items():
            if frag in name:
                seen.add(frag)
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
                vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
                spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
                assert scratch == 0 and spills == 0, f"{name}: {scratch} B of scratch, {spills} spilled VGPRs"
                assert vgprs <= max_vgprs, f"{name}: {vgprs} VGPRs (budget {max_vgprs})"
                if frag in LDS:
                    lds = int(re.search(r"\.amdhsa_kernel\s+" + re.escape(name.replace(".kd", "")) + r"\n(?:.*\n)*?\s+\.amdhsa_group_segment_fixed_size\s+(\d+)", text).group(1))
                    assert lds <= LDS[frag], f"{name}: {lds} B of LDS (budget {LDS[frag]})"
                if frag in MFMA:
                    agprs = int(re.search(r"\.set\s+" + re.escape(name.replace(".kd", "")) + r"\.num_agpr,\s*(\d+)", text).group(1))
                    assert agprs == 0, f"{name}: {agprs} AGPRs: every MFMA result would cost a v_accvgpr_read"
    assert seen == set(HOT[src]), f"kernels not found in {src}: {set(HOT[src]) - seen}"
