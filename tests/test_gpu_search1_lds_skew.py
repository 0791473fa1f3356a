"""The whole-pel search's loop form keeps the current blocks' share of the metric in LDS, a block slot S1_PRE_SLOT = 68 ints apart from the
next (csrc/s1_pre_layout.h: the skew that takes the bank conflicts out of the C reads).  The slot is addressed in two places -- where
s1_make_pre stores it (lane = (slot, sub-block)) and where the cost loop reads it (lane = (slot, dy)) -- and in two kernels: k_search1_pl
(one video) and k_search1_plr_b (a batch, every reference in one workgroup).  Shapes
that put the indexing at its edges, each searched both ways; the level-1 and level-0 nets and the quarter-pel costs that follow from
them must be the CPU oracle's, bit for bit:
    64x48    48 level-0 blocks: exactly one workgroup, every slot of every wave live
    176x144  396 blocks: eight full workgroups and a ninth with one live wave
    208x16   26 blocks: slots 12-15 of s1_make_pre's lane map, dead block slots in the last live wave
At these sizes a launch picks the short-wave form by itself; VP8HIP_S1_SPLIT=0 forces the loop form on every level.  The switch is
read once per process, so this file runs in a process of its own, once for all shapes (the cases below read what it printed).  Run with `pytest -m gpu`."""
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

from oracle_lib import Oracle
from pipeline import default_segments
from vp8oclenc_amd import api
from vp8oclenc_amd.synth import SynthSequence

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (176, 144), (208, 16)]
BATCH_FLAGS = [(0, 0), (1, 1)]      # (use_golden, use_altref) of the batch's two members: one and three enabled references


def _prepare(be, frames):
    """frames[1] GOLDEN, frames[2] ALTREF, frames[0] LAST through the reference's own rotation rules; frames[3] is the current frame"""
    be.upload_last(*frames[1])
    be.upload_current(*frames[3])
    be.inter_transform(1, 0, 0, 0)
    be.loop_filter()
    be.upload_last(*frames[2])
    be.upload_current(*frames[3])
    be.inter_transform(0, 1, 0, 0)
    be.loop_filter()
    be.upload_last(*frames[0])
    be.upload_current(*frames[3])


def _net_differences(tag, hip, ora, flags):
    bad = []
    for r in range(3):
        if r and not flags[r - 1]:
            continue
        for name, got, want in (("level-1 net", hip.debug(api.DBG_NET1, r), ora.net(r, 1)),
                                ("level-0 net", hip.debug(api.DBG_NET2, r), ora.net(r, 2)),
                                ("bdiff", hip.debug(api.DBG_BDIFF, r), ora.bdiff(r))):
            if not np.array_equal(np.asarray(got), np.asarray(want)):
                bad.append((tag, r, name, int((np.asarray(got) != np.asarray(want)).sum())))
    return bad


def _differences(W, H, batch):
    """[(who, reference, what, how many)] where the search's nets are not the oracle's: one video with three references, or the batch"""
    flags = BATCH_FLAGS if batch else [(1, 1)]
    n = len(flags)
    seqs = [SynthSequence(W, H, seed=90 + i) for i in range(n)]
    Wp, Hp = seqs[0].W, seqs[0].H
    sd = default_segments()
    members = [api.Vp8Hip(Wp, Hp) for _ in range(n)]
    oracles = [Oracle(Wp, Hp) for _ in range(n)]
    for i in range(n):
        frames = [seqs[i].frame(t) for t in range(4)]
        for be in (members[i], oracles[i]):
            be.set_segments(sd)
            _prepare(be, frames)
    bad = []
    if batch:
        lib = api.load_library()
        hb = C.c_void_p()
        lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
        lib.vp8hip_batch_inter_transform.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 5
        lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
        lib.vp8hip_batch_destroy.restype = None
        assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * n)(*[m.h for m in members]), n) == 0
        ints = lambda v: (C.c_int * n)(*v)
        assert lib.vp8hip_batch_inter_transform(hb, None, ints([0] * n), ints([0] * n), ints([f[0] for f in flags]), ints([f[1] for f in flags])) == 0
        api.device_synchronize()
    else:
        members[0].inter_transform(0, 0, *flags[0])
    for i, f in enumerate(flags):
        oracles[i].inter_transform(0, 0, *f)
        bad += _net_differences(f"member {i}" if batch else "one video", members[i], oracles[i], f)
    if batch:
        lib.vp8hip_batch_destroy(hb)
    for m in members:
        m.close()
    for o in oracles:
        o.close()
    return bad


def _line(W, H, way):
    return f"{W}x{H} {way}: differences: "


@functools.lru_cache(maxsize=None)
def _child():
    """this file as a program with the loop form forced: its output, once"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, VP8HIP_S1_SPLIT="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("way", ["one video", "batch"], ids=["k_search1_pl", "k_search1_plr_b"])
def test_the_loop_form_with_skewed_block_slots_leaves_the_oracles_nets(way, W, H):
    out = _child()
    assert _line(W, H, way) + "[]" in out, out[-3000:]


if __name__ == "__main__":
    assert os.environ.get("VP8HIP_S1_SPLIT") == "0", "run by the tests above, which force the loop form"
    found = 0
    for W, H in SHAPES:
        for way in ("one video", "batch"):
            bad = _differences(W, H, way == "batch")
            print(_line(W, H, way) + str(bad), flush=True)
            found += len(bad)
    sys.exit(1 if found else 0)
