"""The filled loop form of the batched whole-pel search (k_search1_plr_b) numbers its blocks across the workgroup: 51 blocks x 5 lanes in 256
lanes, lane t = (block slot t / 5, candidate row t % 5), the current blocks' share of the metric in one LDS table of 51 slots of 68 ints made by
the whole workgroup (csrc/s1_fill_layout.h: the map and the addresses the kernel indexes by).  scripts/native/s1_fill_layout_sanitize.cpp walks
that header on the host -- a program of its own, built with the address and undefined-behaviour sanitizers and run as a program:
  * for nblk = 1..400 every block is owned by exactly five lanes (candidate rows 0..4) of exactly one workgroup, no lane addresses a table slot
    >= 51 or a word outside the minimum's buffer, and every slot's 64 ints are made exactly once;
  * the slots whose lanes lie in two waves are 12, 25 and 38;
  * every C read of every wave costs the LDS the four cycles of a conflict-free ds_read_b128 (csrc/lds_bank_model.h) -- and the same table with
    slots of 64 ints does not, so the check can fail.
The row-order A operand of the metric (K_METRIC_A_ROWS, vp8hip_dev.h), which the same kernel multiplies reference rows by, is held here against
metric_w restated in numpy: the per-lane 4x4 byte transpose of the column-order table.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("s1fill") / "s1_fill_layout_sanitize")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + ["-I", os.path.join(ROOT, "vp8oclenc_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "native", "s1_fill_layout_sanitize.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(line.split() for line in r.stdout.splitlines())


def test_every_block_has_five_lanes_of_one_workgroup_and_no_lane_leaves_the_table(figures):
    assert figures["owners_bad"] == "0"
    assert figures["slots_bad"] == "0"
    assert figures["tasks_bad"] == "0"
    assert figures["straddling"] == "12,25,38"
    assert int(figures["lds_bytes"]) <= 16384


def test_every_c_read_of_every_wave_is_conflict_free(figures):
    assert figures["c_stride"] == "68"
    assert figures["c_read"] == "4"       # every wave, sub-block and quad alike (a range would print as lo..hi)


def test_slots_a_bank_row_apart_are_not(figures):
    lo = int(figures["c_read_stride64"].split("..")[0])
    assert lo > 4, figures["c_read_stride64"]


# ---- the row-order operand -------------------------------------------------------------------------------------------
def _pk(*w):
    return [x & 255 for x in w]


R0N, R2N, XN, YN = _pk(-8, -8, 8, -8), _pk(-8, 8, -8, -8), _pk(0, 0, -16, 0), _pk(-32, 0, 0, 32)
R0, R2 = _pk(8, 8, -8, 8), _pk(8, -8, 8, 8)


def _metric_w(i, c):
    """vp8hip_dev.h's metric_w: the weights of quantity i on the four ROWS of prediction column c, as four bytes (the prediction counts negative)"""
    if i >= 8:
        return [0, 0, 0, 0] if (i & 3) != c else (YN if i >= 12 else XN)
    pos, neg = (R0N, R0) if i < 4 else (R2N, R2)
    k = i & 3
    if k == 0:
        return pos
    if k == 1:
        return pos if c in (0, 3) else neg
    if k == 2:
        return pos if c == 1 else neg if c == 2 else [0, 0, 0, 0]
    return pos if c == 0 else neg if c == 3 else [0, 0, 0, 0]


def _weights():
    """W[lane][row r][column c] as bytes: lane l = row m = l & 31 of the block-diagonal A, the half h = l >> 5 that holds it"""
    w = np.zeros((64, 4, 4), np.uint8)
    for l in range(64):
        m, h = l & 31, l >> 5
        if ((m >> 2) & 1) != h:
            continue
        i = (m & 3) + 4 * (m >> 3)
        for c in range(4):
            w[l, :, c] = _metric_w(i, c)
    return w


def test_the_row_order_operand_is_the_per_lane_byte_transpose_of_the_column_order_one():
    from vp8oclenc_amd import api
    lib = api.load_library()
    cols, rows = np.zeros((64, 4), np.uint32), np.zeros((64, 4), np.uint32)
    assert lib.vp8hip_debug_metric_tables(C.c_void_p(cols.ctypes.data), C.c_void_p(rows.ctypes.data)) == 0
    w = _weights()
    cols_b, rows_b = cols.view(np.uint8).reshape(64, 4, 4), rows.view(np.uint8).reshape(64, 4, 4)      # [lane][dword][byte], little endian
    assert np.array_equal(cols_b, w.transpose(0, 2, 1))     # column order: dword c, byte r
    assert np.array_equal(rows_b, w)                        # row order: dword r, byte c
    assert np.array_equal(rows_b, cols_b.transpose(0, 2, 1))
    assert len({tuple(x) for x in rows[np.r_[0:4, 8:12, 16:20, 24:28]].tolist()}) == 16      # the sixteen quantities differ: a transposed index would show
