"""k_overlay_b and k_overlay_prepare, read from the gfx950 code hipcc emits (no GPU needed): no scratch -- the layers of a member's
argument block are indexed by an unrolled loop, and a block indexed by a run-time value is copied to scratch memory without a word
from the compiler -- no spills, no LDS, registers for eight waves per SIMD, and the wide accesses and byte dot products the kernels are
built on."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_overlay_kernels_use_no_scratch_no_lds_and_few_registers(tmp_path):
    out = tmp_path / "k.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "vp8oclenc_amd", "csrc", "kernels_overlay.hip"), "-o", str(out), "-w"], check=True, timeout=600)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:.*\n)*?)\s+\.wavefront_size", text):
        name, body = m.group(1), m.group(2)
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", body).group(1))
        for frag in ("k_overlay_bE", "k_overlay_prepareE"):
            if frag in name:
                seen[frag] = name
                assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0, name
                assert field("vgpr_count") <= 64, f"{name}: {field('vgpr_count')} VGPRs"
    assert set(seen) == {"k_overlay_bE", "k_overlay_prepareE"}, seen

    def code(name):
        return text[text.index(name.replace(".kd", "") + ":"):].split(".amdhsa_kernel")[0]
    frame = code(seen["k_overlay_bE"])
    assert "global_load_dwordx2" in frame and "global_store_dwordx2" in frame and "global_load_dwordx4" in frame      # the frame's rows, T_u and T_v
    assert not re.search(r"v_(rcp|div)_", frame)      # the divisions by 255 are multiplies and shifts
    assert not re.search(r"\bds_", frame)              # no LDS
    prepare = code(seen["k_overlay_prepareE"])
    assert "v_dot4_u32_u8" in prepare and re.search(r"v_dot4c?_i32_i8", prepare) and not re.search(r"\bds_", prepare)
