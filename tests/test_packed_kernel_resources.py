"""The packed-format convert kernels (k_convert_packed_b, kernels_convert.hip) as hipcc emits them for gfx950 (no GPU needed): no
scratch and no spilled registers.  A lane holds two rows of sixteen RGB pixels -- 32 dwords -- at once; an argument block indexed
per lane, or an array the compiler could not keep in registers, would go to scratch memory without a word from the compiler, and a
memory-bound kernel would then read and write its frame twice.  The register counts themselves are reported in DESIGN.md, not bounded."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vp8oclenc_amd", "csrc")
NEW = ["k_convert_packed_bILb0", "k_convert_packed_bILb1"]      # 4:2:2 (YUY2 / UYVY) and RGB (BGRA / RGBA): the matrix and the byte order are arguments


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_packed_convert_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    out = tmp_path / "k.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "kernels_convert.hip"), "-o", str(out), "-w"], check=True, timeout=600)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:.*\n)*?)\s+\.wavefront_size", text):
        name, body = m.group(1), m.group(2)
        for frag in NEW:
            if frag in name:
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
                vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
                spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
                seen[frag] = vgprs
                print(f"{name}: {vgprs} VGPRs, {scratch} B of scratch, {spills} spilled")
                assert scratch == 0 and spills == 0, f"{name}: {scratch} B of scratch, {spills} spilled VGPRs"
    assert set(seen) == set(NEW), f"kernels not found: {set(NEW) - set(seen)}"
    # the vector instructions of each kernel's body, label to .Lfunc_end: the count DESIGN.md section 4 argues from (reported, not bounded)
    for frag in NEW:
        body = re.search(r"^(\S*" + frag + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M).group(2)
        valu, mem = len(re.findall(r"^\s+v_", body, re.M)), len(re.findall(r"^\s+global_", body, re.M))
        print(f"{frag}: {valu} vector instructions, {mem} global loads and stores")
    # the matrix is an argument: four matrices and two byte orders have not become code objects of their own
    assert len(re.findall(r"\.name:\s+\S*k_convert_packed_b\S*\n", text)) == len(NEW)
    # ... and the byte dot products are there
    assert "v_dot4_u32_u8" in text and re.search(r"v_dot4c?_i32_i8", text)
