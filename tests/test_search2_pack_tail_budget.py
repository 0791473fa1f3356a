"""What the batched quarter-pel search issues per (group of eight blocks, reference) with the filter bytes packed without permutes
(round_pack4: the second v_ashr_pk_i8_i32 of a pair writes the upper half of the first one's register) and the result written by the
winning lane (kernels_s2.hip), counted in the gfx950 code hipcc emits (no GPU needed).  Recipe and counting rule:
test_search2_instruction_budget.py, whose loop_valu() is used here -- every `v_*` of a loop's blocks except the MFMAs, counted statically.

    k_search2_b and k_search2_bs      parent    round_pack4 alone    this build
    reference loop                                      443       427                  411
      of which v_perm_b32                               92        76                   76
    once per group of eight blocks                      70        70                   69
    per (group, reference) at three references          466.3     450.3                434.0   (-6.9 %)
    VGPRs                                               72        72                   72

The static count holds more than a wave issues: 19 of the 411 are the `no candidate accepted' result (:1136-1137), which sits behind a
branch that a wave without such a block skips -- 392 issued; the parent's result write was issued by every wave.  (SQ_INSTS_VALU of the
launch in the headline run: -10.9 %, profiles/s2_pack_tail_parent_vs_this.txt.)
The ceilings: the reference loop is the count reached plus 2, as in the other budget files; the permutes, the once-per-group part, the
registers and the scratch are the plan's."""
import os
import re
import shutil
import subprocess

import pytest

from test_search2_instruction_budget import CSRC, REFS, ROOT

REF_LOOP_MAX = 413
PERM_MAX = 76
PER_GROUP_MAX = 80
VGPR_MAX = 72
KERNELS = ["k_search2_bE", "k_search2_bsE"]


def loop_counts(asm_text, kernel_fragment):
    """(VALU of the reference loop, VALU of the group loop, v_perm_b32 of the reference loop, MFMAs) of one kernel, by the rule of
    test_search2_instruction_budget.loop_valu -- restated here because the permutes are counted per loop as well"""
    m = re.search(r"^_Z\w*%s\w*:[^\n]*\n(.*?)\n\s+s_endpgm" % re.escape(kernel_fragment), asm_text, re.M | re.S)
    assert m, f"{kernel_fragment} not found"
    blocks, parent = [], {}          # [innermost loop header or None, valu, mfma, label, perm, parents...]
    cur = None
    for line in m.group(1).split("\n"):
        lab = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", line)
        if lab:
            cur = {"loop": None, "valu": 0, "mfma": 0, "label": lab.group(1), "perm": 0, "parents": []}
            blocks.append(cur)
            line = lab.group(2)
        if cur is None:
            continue
        code = line.split(";")[0].strip()
        note = line[line.index(";"):] if ";" in line else ""
        if not code and note:
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if h:
                cur["loop"] = h.group(1)
            if re.search(r"=>\s*This (Inner )?Loop Header", note):
                cur["loop"] = cur["label"]
            p = re.search(r"Parent Loop (BB\d+_\d+)", note)
            if p:
                cur["parents"].append(p.group(1))
        elif code.startswith("v_mfma"):
            cur["mfma"] += 1
        elif code.startswith("v_"):
            cur["valu"] += 1
            cur["perm"] += code.startswith("v_perm_b32")
    for b in blocks:
        if b["loop"] is not None and b["loop"] == b["label"]:
            parent[b["loop"]] = b["parents"][-1] if b["parents"] else None

    def inside(h, loop):
        while h is not None:
            if h == loop:
                return True
            h = parent.get(h)
        return False
    total_mfma = sum(b["mfma"] for b in blocks)
    sums = {l: tuple(sum(b[k] for b in blocks if inside(b["loop"], l)) for k in ("valu", "mfma", "perm")) for l in parent}
    holding = [l for l in parent if sums[l][1] == total_mfma]
    assert holding, "no loop holds all of the kernel's matrix instructions"
    inner = min(holding, key=lambda l: sums[l][0])
    outer = max(holding, key=lambda l: sums[l][0])
    return sums[inner][0], sums[outer][0], sums[inner][2], total_mfma


def resources(asm_text, kernel_fragment):
    """(NumVgprs, ScratchSize) from the compiler's own summary behind the kernel"""
    m = re.search(r"^_Z\w*%s\w*:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+)" % re.escape(kernel_fragment), asm_text, re.M | re.S)
    assert m, f"no resource summary for {kernel_fragment}"
    return int(m.group(1)), int(m.group(2))


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    out = tmp_path_factory.mktemp("s2") / "k.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "kernels_s2.hip"), "-o", str(out), "-w"], check=True, timeout=600)
    return out.read_text()


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_batched_search_holds_its_count_without_the_permutes_and_with_the_winning_lanes_write(asm, kernel):
    ref_loop, group_loop, perm, mfma = loop_counts(asm, kernel)
    per_group = group_loop - ref_loop
    vgprs, scratch = resources(asm, kernel)
    print(f"{kernel}: reference loop {ref_loop} (parent 443), v_perm_b32 in it {perm} (parent 92), once per group {per_group} (parent 70), per "
          f"(group, reference) at {REFS} references {ref_loop + per_group / REFS:.1f} (parent 466.3); {vgprs} VGPRs, scratch {scratch}")
    assert mfma == 8, mfma
    assert ref_loop <= REF_LOOP_MAX, (ref_loop, REF_LOOP_MAX)
    assert perm <= PERM_MAX, (perm, PERM_MAX)
    assert 0 < per_group <= PER_GROUP_MAX, (per_group, PER_GROUP_MAX)
    assert vgprs <= VGPR_MAX, (vgprs, VGPR_MAX)
    assert scratch == 0, scratch
