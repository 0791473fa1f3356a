"""The quarter-pel search (kernels_s2.hip, search2_body) indexes its three LDS arrays, and makes the small integers of its global addresses, by the
constexpr functions of csrc/s2_lane_layout.h -- each a function of the thread's number alone -- and its reference loop READS what it used to
compute again per reference from a table made of them (K_S2_LANE: 16-bit fields, two to a dword).  scripts/native/s2_lane_layout_check.cpp walks
that header on the host for all 256 threads -- a program of its own, built with the address and undefined-behaviour sanitizers and run as a
program, the arrays real arrays touched through every address:
  * every table field unpacks to the value of its named function and fits its 16 bits;
  * every address lies inside its array, its slot and the part of the slot the kernel gives it; 16-byte accesses are 16-byte aligned;
  * the rule the kernel's LDS reuse rests on: a slot of s_V, s_HT and s_pre is written only by lanes of the wave that owns it (the one wave of
    the fourth-block round writes words 18..25 of every slot's q3, which nobody else writes);
  * the byte ranges the kernel's comment names coincide as stated: the window in the first 512 bytes of the V slot, candidate 25 of 4x4 block 0 at
    bytes 400..415, q3 in words 64..95 of the H slot;
  * every byte of the predictions, of the H array and of the pre table is written as often as the kernel means it to be.
What this does NOT pin: that the named functions equal what the kernel computed before it had them.  The program compares the table, s2_field and
the functions with each other -- one header -- which holds the field order, the packing and the 16-bit fit; that the addresses are the RIGHT ones is
held by the device suites, whose vectors and costs are the oracle's bit for bit (tests/test_gpu_search_lane_table.py and the search suites).
No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("s2lane") / "s2_lane_layout_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + ["-I", os.path.join(ROOT, "vp8oclenc_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "native", "s2_lane_layout_check.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(line.split() for line in r.stdout.splitlines())


def test_every_table_field_unpacks_to_its_function_and_fits_sixteen_bits(figures):
    assert figures["threads"] == "256"
    assert figures["fields_bad"] == "0"
    assert int(figures["fields"]) * 2 <= int(figures["row_bytes"])


def test_every_address_stays_in_its_array_and_sixteen_byte_accesses_are_aligned(figures):
    assert figures["range_bad"] == "0"
    assert figures["align_bad"] == "0"
    assert figures["lds_bytes"] == "22144"


def test_a_slot_is_written_only_by_the_wave_that_owns_it(figures):
    assert figures["owner_bad"] == "0"


def test_the_shared_byte_ranges_coincide_as_the_kernel_says(figures):
    assert figures["overlap_bad"] == "0"
    assert figures["once_bad"] == "0"
