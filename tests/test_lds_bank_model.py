"""The LDS bank rule of the part as a constexpr function (csrc/lds_bank_model.h) and what it says about the C reads of the whole-pel
search's loop form (csrc/s1_pre_layout.h, the address the kernels index by): scripts/native/lds_bank_model.cpp, built here as host code,
prints the LDS cycles of one such ds_read_b128 of a wave.
  * Block slots of 64 ints, as they were: the twelve blocks of a wave queue up on four banks.  The sixty lanes that have a block meet as 5, 6, 6 and
    4 different slots in the read's four lane groups: 21 cycles.  The kernel issues the read for the whole wave, and lanes 60-63, which have
    no block, read slot 0 in the group that held four: 22.
  * The table's stride (68 ints): 4 cycles, a conflict-free read, either way.  kernels_me.hip asserts the same when it is compiled.
k_search2's cost-phase reads are printed by the same program and only recorded (profiles/s1_lds_skew_parent_vs_this.txt).  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("lds") / "lds_bank_model")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "vp8oclenc_amd", "csrc"), os.path.join(ROOT, "scripts", "native", "lds_bank_model.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60)
    print(r.stdout)
    return dict(line.split() for line in r.stdout.splitlines())


def test_block_slots_a_bank_row_apart_cost_the_c_read_21_cycles(figures):
    assert figures["s1_c_stride64_live"] == "21"      # every wave, sub-block and quad alike (a range would print as lo..hi)
    assert figures["s1_c_stride64_wave"] == "22"      # with the four lanes that have no block


def test_the_tables_stride_makes_the_c_read_conflict_free(figures):
    assert figures["s1_stride"] == "68"
    assert figures["s1_c_stride_live"] == "4"
    assert figures["s1_c_stride_wave"] == "4"


def test_the_quarter_pel_searchs_reads_are_reported(figures):
    for j in range(3):
        assert int(figures[f"s2_b_round{j}"]) >= 4     # recorded, not bounded: nothing reads faster than four cycles
        assert f"s2_c_round{j}" in figures
