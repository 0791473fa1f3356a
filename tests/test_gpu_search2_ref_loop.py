"""Quarter-pel search of a batch whose members have one, two and three enabled references: in the batched launch a workgroup takes its
blocks through every enabled reference of ITS context (k_search2_b, k_search2_bs), so members that differ in the number of references
run loops of different lengths side by side in one launch.  Every member's quarter-pel vectors and costs (net_out / bdiff through the
debug taps), its whole-pel vectors and its macroblock results must be the CPU oracle's, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import Oracle
from pipeline import default_segments
from vp8oclenc_amd import api
from vp8oclenc_amd.synth import SynthSequence

pytestmark = pytest.mark.gpu

FLAGS = [(0, 0), (1, 0), (1, 1), (0, 1)]      # (use_golden, use_altref) per member: 1, 2, 3 and 2 references (LAST + ALTREF: a gap in the map)


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


def _differences(W, H):
    """[(member, reference or key, what, how many)] where the batch's results are not the oracle's"""
    n = len(FLAGS)
    seqs = [SynthSequence(W, H, seed=70 + i) for i in range(n)]
    Wp, Hp = seqs[0].W, seqs[0].H
    sd = default_segments()
    lib = api.load_library()
    members = [api.Vp8Hip(Wp, Hp) for _ in range(n)]
    oracles = [Oracle(Wp, Hp) for _ in range(n)]
    for i in range(n):
        frames = [seqs[i].frame(t) for t in range(4)]
        for be in (members[i], oracles[i]):
            be.set_segments(sd)
            _prepare(be, frames)
    hb = C.c_void_p()
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    lib.vp8hip_batch_inter_transform.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 5
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * n)(*[m.h for m in members]), n) == 0
    ints = lambda v: (C.c_int * n)(*v)
    assert lib.vp8hip_batch_inter_transform(hb, None, ints([0] * n), ints([0] * n), ints([f[0] for f in FLAGS]), ints([f[1] for f in FLAGS])) == 0
    api.device_synchronize()
    bad = []
    for i, (use_golden, use_altref) in enumerate(FLAGS):
        oracles[i].inter_transform(0, 0, use_golden, use_altref)
        for r in range(3):
            if r and not (use_golden, use_altref)[r - 1]:
                continue
            for name, got, want in (("net_out", members[i].debug(api.DBG_NET2, r), oracles[i].net(r, 2)),
                                    ("net_1x", members[i].debug(api.DBG_NET1, r), oracles[i].net(r, 1)),
                                    ("bdiff", members[i].debug(api.DBG_BDIFF, r), oracles[i].bdiff(r))):
                if not np.array_equal(np.asarray(got), np.asarray(want)):
                    bad.append((i, r, name, int((np.asarray(got) != np.asarray(want)).sum())))
        a, b = members[i].download_results(recon=True), oracles[i].download_results(recon=True)
        for k in ("MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs", "MB_segment_id"):
            if not np.array_equal(a[k], b[k]):
                bad.append((i, k, "results", int((a[k] != b[k]).sum())))
    lib.vp8hip_batch_destroy(hb)
    for m in members:
        m.close()
    for o in oracles:
        o.close()
    return bad


@pytest.mark.parametrize("W,H", [(320, 192), (176, 144), (648, 360)])
def test_a_batch_whose_members_differ_in_enabled_references_gives_the_oracles_search_results(W, H):
    bad = _differences(W, H)
    assert not bad, f"members with {[1 + sum(f) for f in FLAGS]} references in one batch differ from the oracle: {bad}"
