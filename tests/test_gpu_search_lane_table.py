"""The two batched search kernels after their lane arithmetic moved (quarter-pel search: lane addresses read from K_S2_LANE, csrc/s2_lane_layout.h,
and its three global loads addressed by a uniform base + the lane's unsigned 32-bit offset, the window's base moved back by EXT rows and columns;
whole-pel search: the C reads take a byte address carried in one register, the five candidate keys are made as packed 16-bit pairs), against the CPU oracle, vectors and costs bit for bit, at the shapes the
other suites do not pin for this change.  Through the existing taps: vp8hip_debug_search2_batch, and the child process of test_gpu_search1_fill.py's
machinery (vp8hip_debug_search1_batch with the loop form forced on every level); contents, nets and preparation are that file's and
test_gpu_search2_pack_tail.py's, by import.

Quarter-pel, four members with 1, 2, 3 and 2 (LAST + ALTREF: a gap in the reference map) references in ONE launch:
    16x16     4 blocks: half a group
    48x16    12 blocks, bw = 6: a ragged last group (1.5 groups; a workgroup of two groups half empty), a block row that is no power of two (the
             __umulhi division)
    176x144  396 blocks
  Whole-pel nets that put the window ON each of its four clamp limits and beyond them (3 - EXT and w + EXT - 11 along x, 3 - EXT and h + EXT - 11
  along y, one axis and both): the biased base of the window load meets its smallest lane offset (row 0, column 0 of the moved base) and its
  largest; and nets that put the block on the frame's first and last valid position along each axis (the window then starts 3 samples outside the
  plane and its candidates COUNT: a wrong offset there changes vectors and costs), mixed with in-frame vectors.
Whole-pel, level 0 (and the levels above it where they have a block), loop form forced, members with 1, 2, 3 and 3 references:
    16x16     4 blocks
    64x48    48 blocks: the workgroup three blocks short of full, slots 12, 25 and 38 -- whose five lanes lie in two waves -- occupied
    208x16   52 blocks: one workgroup full and one block over
    272x48   204 = 4 x 51 blocks: exactly full
  with parent vectors at the int16 extremes and at 0 (test_gpu_search1_fill._extreme_net).

What was asked for and cannot be built: 40x24 (15 blocks, bw = 5), 80x40, 136x24 and 104x32 (50, 51, 52 blocks) are no multiples of 16 -- a context
refuses them (vp8hip_create), so a frame's block count is a multiple of 4 and its block row even; the shapes above are the nearest that exist
(ragged group, block row no power of two; 48 / 52 / 204 blocks around a workgroup of 51).  Members of different SIZES cannot share a launch: the
batch and the tap refuse them (one grid for all members; tests/test_gpu_batch_refusals.py).

Before any GPU run, from the nets and the layout alone (no GPU: the first two tests): the clamp cases really clamp, on every limit, and the valid
edge positions are there; the 48-, 52- and 204-block cases really put a block's five lanes in two waves.
Run with `pytest -m gpu`."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

import test_gpu_search1_fill as s1fill
import test_gpu_search2_pack_tail as s2tail
from oracle_lib import Oracle
from pipeline import default_segments
from vp8oclenc_amd import api

EXT = 8                                          # vp8hip_dev.h: the replicated-edge width of a plane
S2_SHAPES = [(16, 16), (48, 16), (176, 144)]
# 4, 48, 52 and 204 blocks.  A frame's block count is a multiple of 4, so "one block short of a full workgroup" (50) and a single workgroup of
# exactly 51 cannot exist: 48 is THREE short, 52 is one over, and the exactly-full case is four workgroups (4 x 51)
S1_SHAPES = [(16, 16), (64, 48), (208, 16), (272, 48)]
FLAGS = s2tail.FLAGS                             # 1, 2, 3 and 2 (a gap in the map) references
LIMITS = ("x low", "x high", "y low", "y high")


def _clamp_net(W, H, seed):
    """a whole-pel net: (b8, 2) int16, cell b = the vector of 8x8 block b.  By b % 8: 0..3 the window ON one clamp limit (origin = the limit itself:
    cx + nx = 3 - EXT or w + EXT - 11, the first position that does not clamp ... ), 4 beyond a limit along both axes, 5 and 6 the frame's first /
    last valid position along both axes, 7 a vector that keeps the block in the frame"""
    rng = np.random.default_rng(seed)
    bw, bh = W // 8, H // 8
    net = np.zeros((bw * bh, 2), np.int16)
    for b in range(bw * bh):
        cx, cy = 8 * (b % bw), 8 * (b // bw)
        lo, hix, hiy = 3 - EXT, W + EXT - 11, H + EXT - 11
        inx, iny = int(rng.integers(-cx, W - 8 - cx + 1)), int(rng.integers(-cy, H - 8 - cy + 1))
        beyond = int(rng.integers(0, 40))
        k = (b + seed) % 8
        if k == 0:
            v = (lo - cx - (beyond if b & 8 else 0), iny)
        elif k == 1:
            v = (hix - cx + (beyond if b & 8 else 0), iny)
        elif k == 2:
            v = (inx, lo - cy - (beyond if b & 8 else 0))
        elif k == 3:
            v = (inx, hiy - cy + (beyond if b & 8 else 0))
        elif k == 4:
            v = ((lo - cx - beyond) if b & 8 else (hix - cx + beyond), (hiy - cy + beyond) if b & 16 else (lo - cy - beyond))
        elif k == 5:
            v = (-cx, -cy)
        elif k == 6:
            v = (W - 8 - cx, H - 8 - cy)
        else:
            v = (inx, iny)
        net[b] = v
    return net


def _clamp_reach(W, H, net):
    """{limit: blocks whose window origin is clamped to it or sits exactly on it}, + the blocks on the first / last valid position, from the net alone"""
    bw = W // 8
    n = {l: 0 for l in LIMITS}
    n.update(on_limit=0, first=0, last=0)
    for b in range(len(net)):
        px, py = 8 * (b % bw) + int(net[b, 0]), 8 * (b // bw) + int(net[b, 1])
        n["x low"] += px <= 3 - EXT
        n["x high"] += px >= W + EXT - 11
        n["y low"] += py <= 3 - EXT
        n["y high"] += py >= H + EXT - 11
        n["on_limit"] += px in (3 - EXT, W + EXT - 11) or py in (3 - EXT, H + EXT - 11)
        n["first"] += (px, py) == (0, 0)
        n["last"] += (px, py) == (W - 8, H - 8)
    return n


@functools.lru_cache(maxsize=None)
def s2_cases(W, H):
    """{(member, reference): (whole-pel net, the oracle's quarter-pel net, the oracle's costs)}, from the CPU oracle alone; computed once per shape"""
    st = Oracle.stages()
    res = {}
    for i, flags in enumerate(FLAGS):
        cur, refs = s2tail._content(W, H, s2tail.CONTENTS[i % 2])      # the panned texture and the noise frame against its inverse
        for r in range(3):
            if not s2tail._use(flags)[r]:
                continue
            net = _clamp_net(W, H, 10 * i + r)
            want = np.zeros_like(net)
            cost = np.zeros(len(net), np.int32)
            st.luma_search_2step(cur, refs[r], net, want, cost, W, H)
            res[(i, r)] = (net, want, cost)
    return res


@pytest.mark.parametrize("W,H", S2_SHAPES)
def test_the_clamp_cases_really_clamp(W, H):
    """on the CPU, from the nets alone: over the members and references of a shape every limit is met, exactly and beyond; the first and last valid
    positions are there; and the blocks that stay in the frame move (their result depends on the window's bytes)"""
    total = {}
    moved = 0
    for (i, r), (net, want, cost) in s2_cases(W, H).items():
        for k, v in _clamp_reach(W, H, net).items():
            total[k] = total.get(k, 0) + int(v)
        moved += int((np.abs(want).sum(axis=1) > 0).sum())
    print(f"{W}x{H}: {total}; blocks with a non-zero quarter-pel vector: {moved}")
    assert all(total[l] > 0 for l in LIMITS), total
    assert total["on_limit"] > 0 and total["first"] > 0 and total["last"] > 0, total
    assert moved > 0


@pytest.mark.parametrize("W,H", S1_SHAPES)
def test_the_block_counts_sit_around_a_full_workgroup(W, H):
    """on the CPU, from the lane map (csrc/s1_fill_layout.h: lane t = block slot t / 5, 51 slots per workgroup of four waves of 64): which occupied
    slots have their five lanes in two waves"""
    nblk = (W // 8) * (H // 8)
    straddling = sorted({s for s in range(min(nblk, 51)) if (5 * s) // 64 != (5 * s + 4) // 64})
    print(f"{W}x{H}: {nblk} blocks = {nblk // 51} full workgroups + {nblk % 51}; occupied slots in two waves: {straddling}")
    assert nblk == {(16, 16): 4, (64, 48): 48, (208, 16): 52, (272, 48): 204}[(W, H)]
    assert straddling == ([] if nblk == 4 else list(s1fill.STRADDLING))
    assert {4: (0, 4), 48: (0, 48), 52: (1, 1), 204: (4, 0)}[nblk] == (nblk // 51, nblk % 51)


def _s2_differences(W, H):
    """[(member, reference, what, how many)] where the tap's results are not the oracle's: the four members in one launch"""
    lib = api.load_library()
    lib.vp8hip_debug_search2_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_void_p)] * 3
    want = s2_cases(W, H)
    n = len(FLAGS)
    members = [api.Vp8Hip(W, H) for _ in FLAGS]
    bad = []
    try:
        for i, m in enumerate(members):
            cur, refs = s2tail._content(W, H, s2tail.CONTENTS[i % 2])
            m.set_segments(default_segments())
            s2tail._prepare(m, cur, refs)
        api.device_synchronize()
        src = {k: np.ascontiguousarray(v[0]) for k, v in want.items()}
        dst = {k: np.full_like(v, 0x3333) for k, v in src.items()}
        cost = {k: np.full(len(v), 0x33333333, np.int32) for k, v in src.items()}
        ptr = lambda d: (C.c_void_p * (3 * n))(*[d[(k, r)].ctypes.data if (k, r) in d else None for k in range(n) for r in range(3)])
        ints = lambda v: (C.c_int * n)(*v)
        rc = lib.vp8hip_debug_search2_batch((C.c_void_p * n)(*[m.h for m in members]), n, ints([f[0] for f in FLAGS]), ints([f[1] for f in FLAGS]),
                                            ptr(src), ptr(dst), ptr(cost))
        assert rc == 0, rc
        for key, (_, wnet, wcost) in want.items():
            for what, got, exp in (("vectors", dst[key], wnet), ("costs", cost[key], wcost)):
                if not np.array_equal(got, exp):
                    bad.append(key + (what, int((got != exp).sum())))
    finally:
        for m in members:
            m.close()
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", S2_SHAPES)
def test_the_quarter_pel_search_on_and_beyond_its_clamp_limits_gives_the_oracles_vectors_and_costs(W, H):
    test_the_clamp_cases_really_clamp(W, H)        # (asserted first, from the CPU alone)
    bad = _s2_differences(W, H)
    assert not bad, bad[:20]


@functools.lru_cache(maxsize=None)
def _child():
    """this file as a program with the whole-pel search's loop form forced on every level: its output, once"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, VP8HIP_S1_SPLIT="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", S1_SHAPES)
def test_the_filled_whole_pel_search_around_a_full_workgroup_gives_the_oracles_vectors(W, H):
    """the level-0 net and what descends from it, and single levels over parent vectors at the int16 extremes and at 0"""
    import re
    test_the_block_counts_sit_around_a_full_workgroup(W, H)
    out = _child()
    assert s1fill._line(W, H) + "[]" in out, out[-3000:]
    levels = [int(l) for l in re.findall(re.escape(f"{W}x{H} extreme parents, level ") + r"(\d)", out)]
    assert 0 in levels, out[-3000:]
    for level in levels:
        m = re.search(re.escape(s1fill._extreme_line(W, H, level)) + r"(\[.*?\]); reach: (\d+) extreme parent components", out)
        assert m and m.group(1) == "[]" and int(m.group(2)) > 0, out[-3000:]


if __name__ == "__main__":
    assert os.environ.get("VP8HIP_S1_SPLIT") == "0", "run by the test above, which forces the loop form"
    found = 0
    for W, H in S1_SHAPES:
        extremes = []
        bad = s1fill._differences(W, H, None, extremes)
        print(s1fill._line(W, H) + str(bad), flush=True)
        found += len(bad)
        for level, ebad, (ext, wrap, far) in extremes:
            print(s1fill._extreme_line(W, H, level) + f"{ebad}; reach: {ext} extreme parent components, {wrap} blocks whose candidates pass int16, "
                  f"{far} vectors out beyond the frame", flush=True)
            found += len(ebad)
    sys.exit(1 if found else 0)
