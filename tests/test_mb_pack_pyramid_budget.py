"""What the macroblock kernel, the pack and the pyramid issue, counted in the gfx950 code hipcc emits with build.py's flags (no GPU needed; the
pattern of test_search2_pack_tail_budget.py).  Every `v_*` instruction of a kernel is counted statically, branches and all.

    kernel                         parent    this build
    k_mb_p                         1624      1479        v_mad_i64_i32 19 -> 3; 122 -> 121 VGPRs
    k_pyramid                      216       173         (the edge rows that share the kernel are untouched and counted in both)
    k_pack_b, copy loop            41 per 8 bytes -> 8 per 16 bytes (4 per 8): the loop is now a lane's 16-byte step along a row

k_mb_p: quantiser division on the signed numerator (three instructions a coefficient), the non-zero count on the packed zig-zag words,
signed saturating pack of the filter sums without the two masks and the bias, the vertical transform's factor 8 folded into constants and
rounding, rows addressed by a 32-bit offset or an addition, and the reconstruction's rows saturated and packed by v_ashr_pk_u8_i32.  The ceilings are the counts reached plus 2, as in the other budget files;
the registers and the scratch are the plan's (four waves per SIMD)."""
import os
import re
import shutil
import subprocess

import pytest

from test_search2_instruction_budget import CSRC, ROOT

MB_P_MAX, MB_P_PARENT = 1481, 1624
MB_P_MAD64_MAX = 3
PYRAMID_MAX, PYRAMID_PARENT = 175, 216
PACK_LOOP_MAX, PACK_LOOP_BYTES, PACK_PARENT_PER_8 = 10, 16, 41
VGPR_MAX = 128

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip", "--cuda-device-only", "-S", "-w"]


def body(asm_text, fragment):
    m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s+s_endpgm" % re.escape(fragment), asm_text, re.M | re.S)
    assert m, f"{fragment} not found"
    return m.group(2)


def valu(text):
    return [c.split()[0] for c in (l.split(";")[0].strip() for l in text.split("\n")) if c.startswith("v_")]


def resources(asm_text, fragment):
    """(NumVgprs, NumAgprs, ScratchSize) from the compiler's own summary behind the kernel"""
    m = re.search(r"^_Z\w*%s\w*:.*?; NumVgprs: (\d+).*?; NumAgprs: (\d+).*?; ScratchSize: (\d+)" % re.escape(fragment), asm_text, re.M | re.S)
    assert m, f"no resource summary for {fragment}"
    return tuple(int(x) for x in m.groups())


def blocks(text):
    """[(loop depth, text)] of a kernel's basic blocks: the depth is what the compiler's loop comments behind the label say (0: in no loop)"""
    out = []
    for part in re.split(r"^(?=\.LBB\d+_\d+:|; %bb\.\d+:)", text, flags=re.M):
        head = []
        for line in part.split("\n")[:4]:
            if ";" in line:
                head.append(line[line.index(";"):])
        d = [int(x) for x in re.findall(r"Depth=(\d+)", " ".join(h for h in head if "Loop" in h))]
        out.append((max(d) if d else 0, part))
    return out


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    d = tmp_path_factory.mktemp("mbpp")
    texts = {}
    for name in ("kernels_mb", "kernels_me"):
        out = d / (name + ".s")
        subprocess.run(["hipcc"] + FLAGS + [os.path.join(CSRC, name + ".hip"), "-o", str(out)], check=True, timeout=600)
        texts[name] = out.read_text()
    return texts


@pytest.mark.parametrize("kernel,ceiling,parent", [("6k_mb_pE", MB_P_MAX, MB_P_PARENT), ("17k_mb_p_conformantE", MB_P_MAX, MB_P_PARENT)])
def test_the_macroblock_kernels_hold_their_count_and_their_registers(asm, kernel, ceiling, parent):
    ops = valu(body(asm["kernels_mb"], kernel))
    vgprs, agprs, scratch = resources(asm["kernels_mb"], kernel)
    mad64 = sum(o.startswith(("v_mad_i64_i32", "v_mad_u64_u32")) for o in ops)
    print(f"{kernel}: {len(ops)} vector instructions (parent {parent}), of which 64-bit multiply-adds {mad64}, v_mul_hi_i32 "
          f"{ops.count('v_mul_hi_i32')}, v_sad_u16 {ops.count('v_sad_u16')}; {vgprs} VGPRs, {agprs} AGPRs, scratch {scratch}")
    assert len(ops) <= ceiling < parent, (len(ops), ceiling)
    assert vgprs <= VGPR_MAX and agprs == 0 and scratch == 0, (vgprs, agprs, scratch)
    assert ops.count("v_mul_hi_i32") >= 17                                          # the division on the signed numerator: 16 + the second-order one
    assert ops.count("v_mul_hi_u32") <= 2                                           # (what is left divides the macroblock number by the frame's width)
    # the filter sums packed signed (six saturated lines + four columns, or all nine lines in the conformant predictor), two instructions each;
    # the reconstruction's four rows unsigned
    assert ops.count("v_ashr_pk_i8_i32") == (26 if "conformant" in kernel else 20) and ops.count("v_ashr_pk_u8_i32") == 8
    if kernel == "6k_mb_pE":
        assert sum(o.startswith("v_mad_i64_i32") for o in ops) <= MB_P_MAD64_MAX


def test_the_pyramid_holds_its_count(asm):
    ops = valu(body(asm["kernels_me"], "9k_pyramidE"))
    vgprs, agprs, scratch = resources(asm["kernels_me"], "9k_pyramidE")
    print(f"k_pyramid: {len(ops)} vector instructions (parent {PYRAMID_PARENT}), v_dot4_u32_u8 {ops.count('v_dot4_u32_u8')}; {vgprs} VGPRs, scratch {scratch}")
    assert len(ops) <= PYRAMID_MAX < PYRAMID_PARENT, len(ops)
    assert ops.count("v_dot4_u32_u8") == 8 and not any(o.startswith("v_bfe_u32") for o in ops)
    assert agprs == 0 and scratch == 0


def test_the_pack_copies_sixteen_bytes_in_a_handful_of_instructions(asm):
    text = body(asm["kernels_me"], "8k_pack_bE")
    vgprs, agprs, scratch = resources(asm["kernels_me"], "8k_pack_bE")
    # the copy loop: the innermost loop's blocks without the byte-wise path (the only blocks with byte loads); one trip = one 16-byte load and store
    inner = [t for d, t in blocks(text) if d == 2]
    assert inner, "no loop of depth 2 in k_pack_b"
    fast = [t for t in inner if "global_load_ubyte" not in t]
    n = sum(len(valu(t)) for t in fast)
    loads = sum(t.count("global_load_dwordx4") for t in fast)
    stores = sum(t.count("global_store_dwordx4") for t in fast)
    print(f"k_pack_b: {n} vector instructions per {PACK_LOOP_BYTES}-byte step of the copy loop = {n * 8 / PACK_LOOP_BYTES:.1f} per 8 bytes "
          f"(parent {PACK_PARENT_PER_8} per 8-byte unit); {vgprs} VGPRs, scratch {scratch}")
    assert loads == 1 and stores == 1, (loads, stores)
    assert 0 < n <= PACK_LOOP_MAX and n * 8 / PACK_LOOP_BYTES < PACK_PARENT_PER_8, n
    assert not any(o.startswith(("v_rcp", "v_mul_hi_u32", "v_mul_lo_u32")) for o in valu(text))      # no division by the row's unit count
    assert agprs == 0 and scratch == 0
