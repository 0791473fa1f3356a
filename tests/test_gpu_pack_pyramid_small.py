"""k_pack_b and k_pyramid (kernels_me.hip) on the smallest frames at which their row and tile structure can go wrong, byte for byte.

Pack: a workgroup owns rows of one plane, a wave a row, a lane 16 bytes -- against the host's padding rule (test_padding.oracle_pad):
    16x16 -> 16x16   nothing to pad; the chroma rows are 8 bytes: half a lane, the row's 8-byte tail and nothing else;
    20x18 -> 32x32   right and bottom padding; tight source rows of 20 and 10 bytes: no row stride is a multiple of 8 (the byte-wise path);
    8x2 -> 16x16     a source narrower than one lane, one chroma row of 4 bytes repeated down the plane;
each with the source planes at 256-byte aligned and at odd addresses, as host planes (packed in place out of the surface), and as a batch
of two members with different frames.

Pyramid: a workgroup takes a 64x64 tile down the four levels -- against a numpy cascade of rounded 2x2 means:
    16x16     a quarter of a tile in both directions: level 4 is one sample;
    80x48     one and a quarter tiles across, three quarters down;
    208x64    three and a quarter tiles, level 4 is 13x4;
on the surface of LAST, whose launch also replicates the edges (border mask on: more rows of workgroups behind the tiles), and on the
current frame's (mask off).  The replicated edge itself is not a thing the C ABI hands out: it is held by the searches of
test_gpu_parity.py, whose windows hang over it.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from pipeline import default_segments
from test_padding import oracle_pad, source
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu

PACK_SIZES = [(16, 16, 16, 16), (20, 18, 32, 32), (8, 2, 16, 16)]


def _surface(hip):
    return [hip.debug(api.DBG_PYRAMID, 3, 0), hip.debug(api.DBG_CURRENT_CHROMA, 0), hip.debug(api.DBG_CURRENT_CHROMA, 1)]


def _to_device(planes, off):
    dev = [api.DeviceBuffer(p.size + 16) for p in planes]
    for d, p in zip(dev, planes):
        d.upload(np.ascontiguousarray(p).reshape(-1), offset=off)
    return dev, [d.data_ptr() + off for d in dev]


@pytest.mark.parametrize("sw,sh,W,H", PACK_SIZES)
def test_pack_pads_like_the_host_rule(sw, sh, W, H):
    hip = api.Vp8Hip(W, H)
    hip.set_source_size(sw, sh)
    for k, (how, off) in enumerate((("host", 0), ("device", 0), ("device at an odd address", 3), ("device at an odd address", 5))):
        src = source(sw, sh, 30 + k)
        exp = oracle_pad(src, W, H)
        if how == "host":
            hip.upload_current(*src)
        else:
            dev, ptrs = _to_device(src, off)
            hip.set_current_device(*ptrs)
        for name, g, e in zip("YUV", _surface(hip), exp):
            assert np.array_equal(g, e), (how, off, name, np.argwhere(g != e)[:4].tolist())
    hip.close()


@pytest.mark.parametrize("sw,sh,W,H", PACK_SIZES)
def test_pack_of_a_batch_of_two_members(sw, sh, W, H):
    lib = api.load_library()
    ctxs = [api.Vp8Hip(W, H) for _ in range(2)]
    hb = C.c_void_p()
    try:
        for m in ctxs:
            m.set_source_size(sw, sh)
        lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
        lib.vp8hip_batch_set_current_device.argtypes = [C.c_void_p, C.POINTER(C.c_int)] + [C.POINTER(C.c_void_p)] * 3
        lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
        lib.vp8hip_batch_destroy.restype = None
        assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * 2)(*[m.h for m in ctxs]), 2) == 0
        srcs = [source(sw, sh, 40), source(sw, sh, 41)]
        held = [_to_device(s, off) for s, off in zip(srcs, (0, 1))]          # the second member's planes at odd addresses
        planes = [(C.c_void_p * 2)(held[0][1][p], held[1][1][p]) for p in range(3)]
        assert lib.vp8hip_batch_set_current_device(hb, None, *planes) == 0
        api.device_synchronize()
        for i, m in enumerate(ctxs):
            for name, g, e in zip("YUV", _surface(m), oracle_pad(srcs[i], W, H)):
                assert np.array_equal(g, e), (i, name, np.argwhere(g != e)[:4].tolist())
    finally:
        if hb:
            lib.vp8hip_batch_destroy(hb)
        for m in ctxs:
            m.close()


def cascade(y):
    """levels 0..4: every level the rounded 2x2 means of the level above (downsample_x2: (a + b + c + d + 2) / 4)"""
    out = [y]
    for _ in range(4):
        a = out[-1].astype(np.int32)
        out.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return out


@pytest.mark.parametrize("W,H", [(16, 16), (80, 48), (208, 64)])
def test_pyramid_is_the_cascade_of_rounded_means_with_and_without_the_edge_rows(W, H):
    last, cur = source(W, H, 50 + W), source(W, H, 51 + W)
    hip = api.Vp8Hip(W, H)
    hip.set_segments(default_segments())
    hip.upload_last(*last)
    hip.upload_current(*cur)
    hip.inter_transform(0, 0, 0, 0)
    for ref, planes, what in ((0, last, "LAST (edge rows in the launch)"), (3, cur, "current (none)")):
        for l, e in enumerate(cascade(planes[0])):
            g = hip.debug(api.DBG_PYRAMID, ref, l)
            assert g.shape == e.shape == (H >> l, W >> l)
            assert np.array_equal(g, e), (what, l, np.argwhere(g != e)[:4].tolist())
    hip.close()
