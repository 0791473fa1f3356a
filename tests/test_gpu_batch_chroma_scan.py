"""vp8hip_batch_chroma_change_async (k_chroma_sad_b, kernels_rc.hip): scene_change()'s two sums for the members of a batch in ONE launch,
the fold riding in it.  Every member's answer is numpy's sum|a - b| // ((W/2)*(H/2)) on the coded chroma of its two current surfaces
(downloaded from the device: padded, scaled and converted as the batched intake left them) and is what the single-context
vp8hip_chroma_change gives on the same frames.  Everything is exact."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_deinterlace import current_surfaces

pytestmark = pytest.mark.gpu
ERR_STATE = -4
MAX_BATCH = 8      # VP8HIP_MAX_BATCH, include/vp8hip_multi.h


class Batch:
    """n contexts of one kind in a vp8hip_batch; take(frames, active) hands every active member its next frame from host memory"""

    def __init__(self, n, coded, setup=None):
        from vp8oclenc_amd import api
        self.m = [api.Vp8Hip(*coded) for _ in range(n)]
        for c in self.m:
            if setup:
                setup(c)
        self.n, self.lib = n, self.m[0].lib
        lib, arr = self.lib, C.POINTER(C.c_void_p)
        lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), arr, C.c_int]
        lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
        lib.vp8hip_batch_destroy.restype = None
        lib.vp8hip_batch_upload_current.argtypes = [C.c_void_p, C.POINTER(C.c_int), arr, arr, arr]
        lib.vp8hip_batch_chroma_change_async.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        self.hb = C.c_void_p()
        assert lib.vp8hip_batch_create(C.byref(self.hb), (C.c_void_p * n)(*[c.h for c in self.m]), n) == 0
        self.chroma = [[] for _ in range(n)]      # the members' coded chroma, frame after frame

    def flags(self, active):
        return None if active is None else (C.c_int * self.n)(*[int(a) for a in active])

    def take(self, frames, active=None):
        on = [active is None or bool(active[i]) for i in range(self.n)]
        planes = [(C.c_void_p * self.n)(*[frames[i][p].ctypes.data if on[i] else None for i in range(self.n)]) for p in range(3)]
        assert self.lib.vp8hip_batch_upload_current(self.hb, self.flags(active), *planes) == 0
        for i, c in enumerate(self.m):
            c.synchronize()
            if on[i]:
                self.chroma[i].append(current_surfaces(c)[1:])

    def scan(self, active=None):
        return self.lib.vp8hip_batch_chroma_change_async(self.hb, self.flags(active))

    def want(self, i):
        """numpy on member i's last two coded frames"""
        (u1, v1), (u0, v0) = self.chroma[i][-1], self.chroma[i][-2]
        nc = u1.size
        return (int(np.abs(u1.astype(np.int64) - u0).sum()) // nc, int(np.abs(v1.astype(np.int64) - v0).sum()) // nc)

    def close(self):
        self.lib.vp8hip_batch_destroy(self.hb)
        for c in self.m:
            c.close()


def i420(rng, w, h, spread, far=False):
    """a random frame whose chroma differs from the next one's by about a third of `spread` per sample (U; V: two thirds); far: by a
    hundred or so from every frame that is not"""
    if far:
        return [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(215, 216 + spread // 2, (h // 2, w // 2), dtype=np.uint8),
                rng.integers(0, 1 + spread // 2, (h // 2, w // 2), dtype=np.uint8)]
    return [rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(100, 101 + spread, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(60, 61 + 2 * spread, (h // 2, w // 2), dtype=np.uint8)]


# coded size, source size (None: the coded size): an 8x8 plane, one workgroup with rows to spare; two row blocks; a source padded on the
# device, 13 row blocks; chroma 1032 wide, the second pass of the x loop
SIZES = [((16, 16), None), ((48, 32), None), ((368, 208), (354, 200)), ((2064, 16), None)]


@pytest.mark.parametrize("n", [1, 3, MAX_BATCH])
@pytest.mark.parametrize("coded,source", SIZES)
def test_the_batch_scan_is_numpy_and_the_single_context_scan(coded, source, n):
    w, h = source or coded
    b = Batch(n, coded, (lambda c: c.set_source_size(w, h)) if source else None)
    rng = np.random.default_rng(coded[0] + n)
    video = [[i420(rng, w, h, 3 + 6 * i, far=t == 2) for t in range(3)] for i in range(n)]      # (the members' differences differ)
    b.take([v[0] for v in video])
    b.take([v[1] for v in video])
    assert b.scan() == 0
    first = [c.chroma_change_result() for c in b.m]
    assert first == [b.want(i) for i in range(n)]
    assert first == [c.chroma_change() for c in b.m]      # the two launches of a context on its own, on the same surfaces
    assert n == 1 or len(set(first)) > 1
    # twice in a row, nothing taken in between: the same answers
    assert b.scan() == 0 and b.scan() == 0
    assert [c.chroma_change_result() for c in b.m] == first
    # the members' videos traded (and a third frame): the answers are the new frames', so the completion counter was back at zero --
    # a counter left standing would never see a last workgroup again, and the words would keep the old sums
    perm = [(i + 1) % n for i in range(n)]
    b.take([video[perm[i]][2] for i in range(n)])
    assert b.scan() == 0
    second = [c.chroma_change_result() for c in b.m]
    assert second == [b.want(i) for i in range(n)] and second != first
    b.close()


def test_members_permuted_give_permuted_results():
    n, (w, h) = 3, (48, 32)
    rng = np.random.default_rng(5)
    video = [[i420(rng, w, h, 4 + 15 * i) for _ in range(2)] for i in range(n)]
    got = {}
    for perm in ((0, 1, 2), (2, 0, 1)):
        b = Batch(n, (w, h))
        for t in range(2):
            b.take([video[perm[i]][t] for i in range(n)])
        assert b.scan() == 0
        got[perm] = [c.chroma_change_result() for c in b.m]
        b.close()
    assert len(set(got[(0, 1, 2)])) == 3
    assert got[(2, 0, 1)] == [got[(0, 1, 2)][p] for p in (2, 0, 1)]


def test_members_sitting_out_and_members_with_one_frame():
    n, (w, h) = 3, (48, 32)
    b = Batch(n, (w, h))
    rng = np.random.default_rng(6)
    f = [[i420(rng, w, h, 20) for _ in range(3)] for _ in range(n)]
    assert b.scan() == ERR_STATE      # no member has a current frame: refused, nothing pending
    for c in b.m:
        assert c.lib.vp8hip_chroma_change_result(c.h, C.byref(C.c_int32()), C.byref(C.c_int32())) == ERR_STATE
    b.take([v[0] for v in f], active=[1, 0, 1])
    assert b.scan(active=[1, 0, 1]) == 0      # one frame each: zeros, and nothing was launched
    assert b.m[0].chroma_change_result() == (0, 0) and b.m[2].chroma_change_result() == (0, 0)
    assert b.scan() == ERR_STATE      # member 1 still has none
    b.take([v[1] for v in f])         # members 0 and 2 have two frames now, member 1 one
    assert b.scan() == 0
    got = [c.chroma_change_result() for c in b.m]
    assert got == [b.want(0), (0, 0), b.want(2)] and got[0] != (0, 0) and got[2] != (0, 0)
    b.take([v[2] for v in f], active=[0, 1, 1])
    assert b.scan(active=[0, 1, 0]) == 0      # member 1 alone; the others' state is not touched
    assert b.m[1].chroma_change_result() == b.want(1) != (0, 0)
    for i in (0, 2):
        assert b.m[i].lib.vp8hip_chroma_change_result(b.m[i].h, C.byref(C.c_int32()), C.byref(C.c_int32())) == ERR_STATE
    # a pending answer survives the batch (its stream is synchronised when it goes)
    assert b.scan() == 0
    want = [b.want(i) for i in range(n)]
    b.lib.vp8hip_batch_destroy(b.hb)
    assert [c.chroma_change_result() for c in b.m] == want
    for c in b.m:
        c.close()


@pytest.mark.parametrize("n", [1, MAX_BATCH])
def test_zero_against_255_is_exactly_255(n):
    w, h = 48, 32
    b = Batch(n, (w, h))
    lo = [np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.full((h // 2, w // 2), 255, np.uint8)]
    hi = [np.zeros((h, w), np.uint8), np.full((h // 2, w // 2), 255, np.uint8), np.zeros((h // 2, w // 2), np.uint8)]
    b.take([lo] * n)
    b.take([hi] * n)
    assert b.scan() == 0
    assert [c.chroma_change_result() for c in b.m] == [(255, 255)] * n
    b.close()


def test_through_the_scaler():
    """112x80 frames scaled to 56x40 in a coded frame of 64x48: the sums are those of the scaled, padded surfaces"""
    b = Batch(2, (64, 48), lambda c: c.set_source_scaling(112, 80, 56, 40))
    rng = np.random.default_rng(8)
    for t in range(2):
        b.take([i420(rng, 112, 80, 30 + 40 * i) for i in range(2)])
    assert b.scan() == 0
    got = [c.chroma_change_result() for c in b.m]
    assert got == [b.want(0), b.want(1)] == [c.chroma_change() for c in b.m] and got[0] != got[1] and (0, 0) not in got
    b.close()


def test_through_the_nv12_converter():
    """NV12 frames of 44x30 in a coded frame of 48x32: the sums are those of the converted, padded surfaces"""
    w, h = 44, 30
    b = Batch(2, (48, 32), lambda c: (c.set_source_size(w, h), c.set_source_format("nv12")))
    rng = np.random.default_rng(9)
    for t in range(2):
        frames = []
        for i in range(2):
            y, u, v = i420(rng, w, h, 25 + 50 * i)
            uv = np.ascontiguousarray(np.stack([u, v], axis=-1).reshape(h // 2, w))
            frames.append([y, uv, uv])      # (the third pointer is never read)
        b.take(frames)
    assert b.scan() == 0
    got = [c.chroma_change_result() for c in b.m]
    assert got == [b.want(0), b.want(1)] == [c.chroma_change() for c in b.m] and got[0] != got[1] and (0, 0) not in got
    b.close()
