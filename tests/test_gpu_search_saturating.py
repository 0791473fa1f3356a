"""The whole motion search on content that saturates the block-match metric: frames of random 0 / 255 squares of 1, 2 and 4 pixels, and
a frame of single pixels against its inverse.  Every difference is 0 or +-255, so the quantities the folded metric takes out of its
matrix instruction (weight_mfma, vp8hip_dev.h) run at their bounds and the costs of an 8x8 block climb past 0x4000, into the upper half of
what the ushort accumulator of the whole-pel search and the 0x7fff acceptance limit of both searches let through.  The members of a batch
have 1, 2, 3 and 2 references (as in test_gpu_search2_ref_loop.py), and one context runs un-batched with three references, for the
one-video forms of the kernels.  Whole-pel vectors, quarter-pel vectors and costs (the debug taps) and the macroblock results must be the
CPU oracle's, bit for bit.

What the content reaches, from the oracle on the CPU (checked before anything runs on the device).  A search keeps the CHEAPEST of its
candidates, so the winning costs (bdiff) stay low: at most 12768 at 80x48 and 12048 at 176x144.  The costs the kernels have to get right
are the candidates': the zero-vector candidate against LAST -- one of the 26 of the quarter-pel search -- costs up to 23392 (0x5b60) at
80x48, 122 of the 300 blocks above 0x4000, and up to 24577 (0x6001) at 176x144, 815 of 1980 above 0x4000.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import Oracle
from pipeline import default_segments
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu

FLAGS = [(0, 0), (1, 0), (1, 1), (0, 1)]      # (use_golden, use_altref) per member: 1, 2, 3 and 2 references
SOLO = (1, 1)                                 # the un-batched context: three references


def _binary(rng, W, H, px):
    """a frame of random 0 / 255 squares of px pixels (luma; chroma the same at half the size)"""
    def plane(w, h):
        cells = rng.integers(0, 2, size=((h + px - 1) // px, (w + px - 1) // px), dtype=np.uint8) * 255
        return np.ascontiguousarray(np.kron(cells, np.ones((px, px), np.uint8))[:h, :w])
    return plane(W, H), plane(W // 2, H // 2), plane(W // 2, H // 2)


def _frames(W, H):
    """per context four frames (GOLDEN, ALTREF, LAST sources and the current one): members 0..2 squares of 1, 2 and 4 pixels; member 3 and
    the un-batched context a frame of single pixels against its inverse (the current frame is 255 - LAST: every difference at the zero
    vector is +-255)"""
    rng = np.random.default_rng(1000 + W)
    out = []
    for px in (1, 2, 4, 1, 1):
        out.append([_binary(rng, W, H, px) for _ in range(4)])
    for i in (3, 4):
        out[i][3] = tuple(255 - p for p in out[i][0])
    return out


def _zero_vector_costs(W, H):
    """the cost of every 8x8 block's zero-vector candidate against LAST (a candidate of both searches), from the oracle's metric on the CPU"""
    lib = Oracle.lib()
    costs = []
    for frames in _frames(W, H):
        d = frames[3][0].astype(np.int32) - frames[0][0].astype(np.int32)
        for by in range(0, H, 8):
            for bx in range(0, W, 8):
                costs.append(sum(lib.vp8o_weight(np.ascontiguousarray(d[by + sy:by + sy + 4, bx + sx:bx + sx + 4]).reshape(16))
                                 for sy in (0, 4) for sx in (0, 4)))
    return np.array(costs)


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


def _oracle_results(W, H):
    """per context: ({(reference, what): array}, macroblock results), from the CPU oracle alone"""
    res = []
    sd = default_segments()
    for frames, (use_golden, use_altref) in zip(_frames(W, H), FLAGS + [SOLO]):
        o = Oracle(W, H)
        o.set_segments(sd)
        _prepare(o, frames)
        o.inter_transform(0, 0, use_golden, use_altref)
        nets = {}
        for r in range(3):
            if r and not (use_golden, use_altref)[r - 1]:
                continue
            nets[(r, "net_1x")] = np.array(o.net(r, 1))
            nets[(r, "net_out")] = np.array(o.net(r, 2))
            nets[(r, "bdiff")] = np.array(o.bdiff(r))
        res.append((nets, {k: np.array(v) for k, v in o.download_results(recon=True).items()}))
        o.close()
    return res


_cache = {}


def oracle_results(W, H):
    if (W, H) not in _cache:
        _cache[(W, H)] = _oracle_results(W, H)
    return _cache[(W, H)]


def _compare(member, idx, flags, want, bad):
    nets, mb = want
    for r in range(3):
        if r and not flags[r - 1]:
            continue
        for name, tap in (("net_out", api.DBG_NET2), ("net_1x", api.DBG_NET1), ("bdiff", api.DBG_BDIFF)):
            got = np.asarray(member.debug(tap, r))
            if not np.array_equal(got, nets[(r, name)]):
                bad.append((idx, r, name, int((got != nets[(r, name)]).sum())))
    a = member.download_results(recon=True)
    for k in ("MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs", "MB_segment_id", "prefilter_Y", "prefilter_U", "prefilter_V"):
        if not np.array_equal(a[k], mb[k]):
            bad.append((idx, k, "results", int((a[k] != mb[k]).sum())))
    x, y = np.asarray(a["MB_SSIM"], np.float32).view(np.uint32), np.asarray(mb["MB_SSIM"], np.float32).view(np.uint32)
    if not np.array_equal(x, y):      # by bit pattern: the value gates the segment loop
        bad.append((idx, "MB_SSIM", "results", int((x != y).sum())))


@pytest.mark.parametrize("W,H", [(80, 48), (176, 144)])
def test_the_search_on_saturating_content_gives_the_oracles_results_batched_and_unbatched(W, H):
    want = oracle_results(W, H)
    # on the CPU first: the content does what it is here for
    zc = _zero_vector_costs(W, H)
    won = max(int(v.max()) for nets, _ in want for (r, name), v in nets.items() if name == "bdiff")
    print(f"{W}x{H}: largest cost of a zero-vector candidate {int(zc.max())} ({int(zc.max()):#x}), {int((zc > 0x4000).sum())} of {zc.size} blocks above "
          f"0x4000; largest winning cost {won}")
    assert zc.max() > 0x4000, int(zc.max())

    n = len(FLAGS)
    all_frames = _frames(W, H)
    sd = default_segments()
    lib = api.load_library()
    members = [api.Vp8Hip(W, H) for _ in range(n + 1)]      # the last one runs un-batched
    bad = []
    hb = C.c_void_p()
    try:
        for m, frames in zip(members, all_frames):
            m.set_segments(sd)
            _prepare(m, frames)
        lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
        lib.vp8hip_batch_inter_transform.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 5
        lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
        lib.vp8hip_batch_destroy.restype = None
        assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * n)(*[m.h for m in members[:n]]), n) == 0
        ints = lambda v: (C.c_int * n)(*v)
        assert lib.vp8hip_batch_inter_transform(hb, None, ints([0] * n), ints([0] * n), ints([f[0] for f in FLAGS]), ints([f[1] for f in FLAGS])) == 0
        api.device_synchronize()
        for i in range(n):
            _compare(members[i], i, FLAGS[i], want[i], bad)
        members[n].inter_transform(0, 0, *SOLO)
        _compare(members[n], "un-batched", SOLO, want[n], bad)
    finally:
        if hb:
            lib.vp8hip_batch_destroy(hb)
        for m in members:
            m.close()
    assert not bad, f"search results on saturating content differ from the oracle: {bad}"
