"""What a wave of the batched quarter-pel search issues per (group of eight blocks, reference), counted in the gfx950 code hipcc emits
(no GPU needed).  The search kernels are bound by vector-instruction issue, so this count is what the kernel costs.

Method: kernels_s2.hip is compiled to assembly with the flags of test_kernel_resources.py.  The basic blocks of k_search2_b
(SPREAD, two groups per workgroup: the form batches run) are assigned to loops by the compiler's own annotations (`=>This Loop Header`,
`Parent Loop`, `in Loop: Header=`), not by their place in the text.  The reference loop is the innermost loop that holds all eight of
the kernel's matrix instructions (the two passes 4, the metric 3 + the fourth-block round), the group loop the outermost one around it.
VALU = every `v_*` instruction of a loop's blocks and of the loops nested in it, v_mfma_* excluded, counted statically: the
fourth-block round, which one wave in four runs, and the writing lane's tail count in full.  Per (group, reference) at three
references = the reference loop + (the group loop - the reference loop) / 3.

    parent commit (one reference per grid y, k_search2_b<true, 4>: one loop, the whole body)       522
    this build: reference loop 475, once-per-group part 53                                         492.7   (-5.6 %)

The change was expected to show at least 8 % (480); it shows 5.6 %: the reference-independent part of the body was smaller than the
estimate it was planned on, and a third of it is still paid per reference.  The ceiling is the parent's count less the margin this
change did achieve.  The register / LDS pins of every k_search2* form stay in test_kernel_resources.py (no kernel changed its name)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vp8oclenc_amd", "csrc")
PARENT_VALU = 522      # loop_valu() on the parent commit's kernels_s2.hip, k_search2_b<true, 4>: (522, 522, 8)
CEILING = 493
REFS = 3


def loop_valu(asm_text, kernel_fragment):
    """(VALU of the innermost loop that holds every MFMA of the kernel, VALU of the outermost loop around it, MFMAs), from the
    compiler's own loop annotations on the basic blocks"""
    m = re.search(r"^_Z\w*%s\w*:[^\n]*\n(.*?)\n\s+s_endpgm" % re.escape(kernel_fragment), asm_text, re.M | re.S)
    assert m, f"{kernel_fragment} not found"
    blocks, parent = [], {}          # [innermost loop header or None, valu, mfma]; loop header -> parent loop header
    cur = None
    for line in m.group(1).split("\n"):
        lab = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", line)
        if lab:
            cur = [None, 0, 0, lab.group(1)]
            blocks.append(cur)
            line = lab.group(2)
        if cur is None:
            continue
        code = line.split(";")[0].strip()
        note = line[line.index(";"):] if ";" in line else ""
        if not code and note:                                   # the block's annotations: its label's line and the comment lines behind it
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if h:
                cur[0] = h.group(1)
            if re.search(r"=>\s*This (Inner )?Loop Header", note):
                cur[0] = cur[3]
            p = re.search(r"Parent Loop (BB\d+_\d+)", note)
            if p:
                cur.append(p.group(1))
        elif code.startswith("v_mfma"):
            cur[2] += 1
        elif code.startswith("v_"):
            cur[1] += 1
    for b in blocks:
        if b[0] == b[3] and b[0] is not None:
            ps = b[4:]
            parent[b[0]] = ps[-1] if ps else None               # (the innermost parent is listed last among the Parent Loop lines)
    def inside(h, loop):                                        # is loop h `loop` or nested in it
        while h is not None:
            if h == loop:
                return True
            h = parent.get(h)
        return False
    total_mfma = sum(b[2] for b in blocks)
    sums = {l: (sum(b[1] for b in blocks if inside(b[0], l)), sum(b[2] for b in blocks if inside(b[0], l))) for l in parent}
    holding = [l for l in parent if sums[l][1] == total_mfma]
    assert holding, "no loop holds all of the kernel's matrix instructions"
    inner = min(holding, key=lambda l: sums[l][0])
    outer = max(holding, key=lambda l: sums[l][0])
    return sums[inner][0], sums[outer][0], total_mfma


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_batched_search_stays_under_its_vector_instruction_ceiling_per_group_and_reference(tmp_path):
    out = tmp_path / "k.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "kernels_s2.hip"), "-o", str(out), "-w"], check=True, timeout=600)
    ref_loop, group_loop, mfma = loop_valu(out.read_text(), "k_search2_bE")
    assert mfma == 8, f"{mfma} matrix instructions in the kernel (the two passes 4, the metric 3 + the fourth-block round)"
    assert group_loop > ref_loop, "no reference loop inside the group loop"
    per_group_ref = ref_loop + (group_loop - ref_loop) / REFS
    print(f"VALU per wave: reference loop {ref_loop}, once per group {group_loop - ref_loop}, per (group, reference) at {REFS} references "
          f"{per_group_ref:.1f} (parent {PARENT_VALU}: {100 * (1 - per_group_ref / PARENT_VALU):.1f} % fewer)")
    assert per_group_ref <= CEILING, f"{per_group_ref:.1f} VALU per (group, reference), ceiling {CEILING} (parent {PARENT_VALU})"
