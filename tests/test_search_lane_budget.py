"""What the two search kernels issue around the metric, with the quarter-pel search's lane addresses read from a table (csrc/s2_lane_layout.h,
K_S2_LANE), its three global loads addressed by a uniform base and a 32-bit lane offset, and the whole-pel search's C reads taking their byte
address from the one register that carries it -- counted in the gfx950 code hipcc emits (no GPU needed).  Recipe and counting rule:
test_search2_instruction_budget.py (loop_valu) and test_search2_pack_tail_budget.py (loop_counts, resources), used here by import.

The PARENT commit's code objects, counted with the same functions:

    k_search2_b, k_search2_bs     parent    this build
    reference loop                                  411       371
    once per group of eight blocks                  69        75
    VGPRs                                           72        69
    LDS bytes                                       22144 / 22180 (with the scans' words)   the same
    k_search1_plr_b
    sub-block loop                                  351       341
    reference loop                                  501       455
    VGPRs                                           68        62
    LDS bytes                                       15952     the same

The bars: the quarter-pel reference loop at most the parent's - 30 with no 64-bit address arithmetic and no 32-bit multiply left in it; the
whole-pel sub-block loop at most the parent's - 5 with no v_lshlrev_b32 in it; registers not above the parent's, no scratch, LDS unchanged.
With the five candidate keys of the whole-pel search's tail as packed 16-bit pairs: the reference loop at most the parent's - 4 x 5 - 25 = 456
(reached: 455; the tail behind the sub-block loop 150 -> 114)."""
import os
import re
import shutil
import subprocess

import pytest

from test_search2_instruction_budget import CSRC, ROOT, loop_valu
from test_search2_pack_tail_budget import loop_counts, resources

# loop_counts / loop_valu / resources on the parent commit's kernels_s2.hip and kernels_me.hip
PARENT_S2_REF_LOOP = 411
PARENT_S2_VGPRS = 72
PARENT_S2_LDS = {"k_search2_bE": 22144, "k_search2_bsE": 22180}
PARENT_S1_SUB_LOOP = 351
PARENT_S1_REF_LOOP = 501
PARENT_S1_VGPRS = 68
PARENT_S1_LDS = 15952
S2_KERNELS = ["k_search2_bE", "k_search2_bsE"]
S2_FORBIDDEN = ("v_mad_i64_i32", "v_lshl_add_u64", "v_mul_lo_u32", "v_mov_b64")


def _compile(tmp, name):
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    out = tmp / (name + ".s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(CSRC, name + ".hip"), "-o", str(out), "-w"], check=True, timeout=600)
    return out.read_text()


@pytest.fixture(scope="module")
def asm_s2(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("lane_s2"), "kernels_s2")


@pytest.fixture(scope="module")
def asm_me(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("lane_me"), "kernels_me")


def loop_opcodes(asm_text, kernel_fragment, want_mfma):
    """opcode -> count over the blocks of the innermost loop that holds `want_mfma` matrix instructions (the compiler's own loop annotations, as in
    loop_valu: the reference loop of the quarter-pel search holds all 8, the sub-block loop of the whole-pel search all 5)"""
    m = re.search(r"^_Z\w*%s\w*:[^\n]*\n(.*?)\n\s+s_endpgm" % re.escape(kernel_fragment), asm_text, re.M | re.S)
    assert m, f"{kernel_fragment} not found"
    blocks, parent, cur = [], {}, None
    for line in m.group(1).split("\n"):
        lab = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", line)
        if lab:
            cur = {"loop": None, "label": lab.group(1), "ops": [], "parents": []}
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
        elif code:
            cur["ops"].append(code.split()[0])
    for b in blocks:
        if b["loop"] is not None and b["loop"] == b["label"]:
            parent[b["loop"]] = b["parents"][-1] if b["parents"] else None

    def inside(h, loop):
        while h is not None:
            if h == loop:
                return True
            h = parent.get(h)
        return False
    ops = {l: [o for b in blocks if inside(b["loop"], l) for o in b["ops"]] for l in parent}
    holding = [l for l in parent if sum(o.startswith("v_mfma") for o in ops[l]) == want_mfma]
    assert holding, f"no loop with {want_mfma} matrix instructions"
    inner = min(holding, key=lambda l: len(ops[l]))
    count = {}
    for o in ops[inner]:
        count[o] = count.get(o, 0) + 1
    return count


def lds_bytes(asm_text, kernel_fragment):
    m = re.search(r"\.amdhsa_kernel _Z\w*%s\w*\n(.*?)\.end_amdhsa_kernel" % re.escape(kernel_fragment), asm_text, re.S)
    assert m, f"{kernel_fragment}'s kernel descriptor not found"
    return int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(1)).group(1))


@pytest.mark.parametrize("kernel", S2_KERNELS)
def test_the_quarter_pel_reference_loop_reads_its_lane_addresses(asm_s2, kernel):
    ref_loop, group_loop, _, mfma = loop_counts(asm_s2, kernel)
    vgprs, scratch = resources(asm_s2, kernel)
    ops = loop_opcodes(asm_s2, kernel, 8)
    left = {o: n for o, n in ops.items() if o.startswith(S2_FORBIDDEN)}
    print(f"{kernel}: reference loop {ref_loop} (parent {PARENT_S2_REF_LOOP}), once per group {group_loop - ref_loop}, {vgprs} VGPRs (parent "
          f"{PARENT_S2_VGPRS}), scratch {scratch}, LDS {lds_bytes(asm_s2, kernel)}; 64-bit address arithmetic and 32-bit multiplies left in the loop: {left}")
    assert mfma == 8, mfma
    assert ref_loop <= PARENT_S2_REF_LOOP - 30, (ref_loop, PARENT_S2_REF_LOOP)
    assert not left, left
    assert vgprs <= PARENT_S2_VGPRS, (vgprs, PARENT_S2_VGPRS)
    assert scratch == 0, scratch
    assert lds_bytes(asm_s2, kernel) == PARENT_S2_LDS[kernel]


def test_the_whole_pel_sub_block_loop_reads_c_without_a_shift_per_candidate(asm_me):
    sub_loop, ref_loop, mfma = loop_valu(asm_me, "k_search1_plr_b")
    vgprs, scratch = resources(asm_me, "k_search1_plr_b")
    ops = loop_opcodes(asm_me, "k_search1_plr_b", 5)
    shifts = sum(n for o, n in ops.items() if o.startswith("v_lshlrev_b32"))
    moves = sum(n for o, n in ops.items() if o.startswith("v_mov_b32"))
    print(f"k_search1_plr_b: sub-block loop {sub_loop} (parent {PARENT_S1_SUB_LOOP}), reference loop {ref_loop}, {vgprs} VGPRs (parent {PARENT_S1_VGPRS}), "
          f"scratch {scratch}, LDS {lds_bytes(asm_me, 'k_search1_plr_b')}; in the sub-block loop {shifts} v_lshlrev_b32, {moves} v_mov_b32, "
          f"{ops.get('ds_read_b128', 0)} ds_read_b128")
    assert mfma == 5, mfma
    assert sub_loop <= PARENT_S1_SUB_LOOP - 5, (sub_loop, PARENT_S1_SUB_LOOP)
    assert shifts == 0, shifts
    assert ref_loop <= PARENT_S1_REF_LOOP - 4 * 5 - 25, (ref_loop, PARENT_S1_REF_LOOP)      # the packed candidate keys
    assert moves <= 5, moves              # at most one per candidate
    assert ops.get("ds_read_b128", 0) == 20, ops.get("ds_read_b128", 0)     # the C input is still read per candidate: four reads each
    assert vgprs <= PARENT_S1_VGPRS, (vgprs, PARENT_S1_VGPRS)
    assert scratch == 0, scratch
    assert lds_bytes(asm_me, "k_search1_plr_b") == PARENT_S1_LDS
