"""The window and the orientation of source frames without a GPU: vp8host_source_window against the table of include/vp8hip_host.h
typed again in tests/geometry_ref.py, every refusal, vp8host_window_frame against numpy slicing, vp8host_orient_frame against
np.rot90 and [:, ::-1], the identities, and the ABI: new entry points, vp8drv_config and the ABI version unchanged.
tests/test_gpu_geometry.py holds the kernels to the same restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geometry_ref as ref
from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = sorted(ref.TABLE)
NEW_SYMBOLS = ["vp8hip_set_source_window", "vp8hip_set_source_orientation", "vp8host_source_window", "vp8host_window_frame",
               "vp8host_orient_frame", "vp8drv_set_source_window", "vp8drv_set_source_orientation"]
SURFACE = (80, 48)
WINDOW = (48, 32)


def test_the_table_has_all_twelve_formats():
    assert len(FORMATS) == 12
    assert FORMATS == list(range(api.FORMAT_I420, api.FORMAT_I410 + 1)) + [api.FORMAT_YUY2, api.FORMAT_UYVY, api.FORMAT_BGRA, api.FORMAT_RGBA]


@pytest.mark.parametrize("fmt", FORMATS)
def test_source_window_is_the_table(fmt):
    for w, h in (WINDOW, (50, 36), (2, 2)):
        nb = api.source_plane_bytes(fmt, w, h)
        for x, y in ref.ORIGINS:
            for extra in ref.EXTRA_PITCH:
                pitch = [p + extra for p in ref.tight_pitch(fmt, x + w + 16)] + [0, 0]      # (entries of planes the format lacks: ignored)
                off, rb, rows = api.source_window(fmt, w, h, x, y, pitch[:3])
                for p in range(3):
                    if p >= len(ref.TABLE[fmt]):
                        assert (off[p], rb[p], rows[p]) == (0, 0, 0) and nb[p] == 0
                        continue
                    hs, vs, bpe = ref.TABLE[fmt][p]
                    assert rows[p] == h >> vs and rb[p] == (w >> hs) * bpe
                    assert off[p] == (y >> vs) * pitch[p] + (x >> hs) * bpe
                    assert rows[p] * rb[p] == nb[p]


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_refusal(fmt):
    w, h = WINDOW
    tight = ref.tight_pitch(fmt, SURFACE[0]) + [0, 0]
    tight = tight[:3]
    assert api.source_window(fmt, w, h, 0, 0, tight)
    for x, y in ((-2, 0), (0, -2), (1, 0), (0, 1), (3, 5)):
        with pytest.raises(ValueError):
            api.source_window(fmt, w, h, x, y, tight)
    for bw, bh in ((0, 32), (48, 0), (47, 32), (48, 31), (-48, 32)):
        with pytest.raises(ValueError):
            api.source_window(fmt, bw, bh, 0, 0, tight)
    api.source_window(fmt, w, h, SURFACE[0] - w, 0, tight)      # the window ends with the row: legal
    with pytest.raises(ValueError):
        api.source_window(fmt, w, h, SURFACE[0] - w + 2, 0, tight)
    for p, (hs, _, bpe) in enumerate(ref.TABLE[fmt]):              # one byte short in any one plane the format has
        for x in (0, 14):
            need = ((x + w) >> hs) * bpe
            pitch = [max(t, need) for t in tight]
            pitch[p] = need
            assert ref.valid(fmt, w, h, x, 2, pitch)
            api.source_window(fmt, w, h, x, 2, pitch)
            pitch[p] = need - 1
            assert not ref.valid(fmt, w, h, x, 2, pitch)
            with pytest.raises(ValueError):
                api.source_window(fmt, w, h, x, 2, pitch)
    for p in range(len(ref.TABLE[fmt]), 3):                          # a plane the format lacks: its pitch is not looked at
        pitch = list(tight)
        pitch[p] = -5
        api.source_window(fmt, w, h, 0, 0, pitch)
    with pytest.raises(ValueError):
        api.source_window(9, w, h, 0, 0, tight)                      # 8 .. 15 are no format
    lib = api.load_library()
    lib.vp8host_source_window.argtypes = [C.c_int] * 5 + [C.c_void_p] * 4
    three = (C.c_size_t * 3)()
    assert lib.vp8host_source_window(fmt, w, h, 0, 0, None, three, three, three) == -1


@pytest.mark.parametrize("fmt", FORMATS)
def test_window_frame_is_numpy_slicing(fmt):
    rng = np.random.default_rng(100 + fmt)
    (sw, sh), (w, h) = SURFACE, WINDOW
    for extra in ref.EXTRA_PITCH:
        pitch = [p + extra for p in ref.tight_pitch(fmt, sw)]
        planes = ref.surface(fmt, sw, sh, pitch, rng)
        for x, y in ref.ORIGINS:
            want = ref.window(fmt, planes, w, h, x, y)
            got = api.window_frame(fmt, w, h, x, y, pitch, planes)
            assert len(got) == len(want)
            for g, t in zip(got, want):
                assert np.array_equal(g, t.ravel()), (fmt, extra, x, y)
            assert [g.size for g in got] == [n for n in api.source_plane_bytes(fmt, w, h) if n]


@pytest.mark.parametrize("size", [(50, 36), (36, 70), (16, 16), (2, 2)])      # chroma 25 wide (odd); chroma 35 high (odd)
@pytest.mark.parametrize("turns,mirror", ref.ORIENTATIONS)
def test_orient_frame_is_rot90_behind_a_flip(size, turns, mirror):
    f = ref.raw_frame(*size, seed=turns * 2 + mirror)
    got = api.orient_frame(turns, mirror, f)
    for g, p in zip(got, f):
        s = p[:, ::-1] if mirror else p
        want = {0: s, 1: np.rot90(s, -1), 2: s[::-1, ::-1], 3: np.rot90(s, 1)}[turns]
        assert g.shape == want.shape and np.array_equal(g, want)
    for g, t in zip(got, ref.orient(f, turns, mirror)):
        assert np.array_equal(g, t)
    if turns & 1:
        assert got[0].shape == (size[0], size[1])      # rows = the raw width
    # the formulas of the header, sample by sample, on the luma plane
    rw, rh = size
    s = (lambda x, y: f[0][y, rw - 1 - x]) if mirror else (lambda x, y: f[0][y, x])
    rule = {0: lambda x, y: s(x, y), 1: lambda x, y: s(y, rh - 1 - x), 2: lambda x, y: s(rw - 1 - x, rh - 1 - y), 3: lambda x, y: s(rw - 1 - y, x)}[turns]
    oh, ow = got[0].shape
    for x, y in ((0, 0), (ow - 1, 0), (0, oh - 1), (ow - 1, oh - 1), (ow // 2, oh // 3)):
        assert got[0][y, x] == rule(x, y)


def test_identities():
    f = ref.raw_frame(50, 36, seed=5)
    same = lambda a, b: all(np.array_equal(p, q) for p, q in zip(a, b))
    assert same(api.orient_frame(0, 0, f), f)
    assert same(api.orient_frame(3, 0, api.orient_frame(1, 0, f)), f)      # turns 1 then 3
    assert same(api.orient_frame(0, 1, api.orient_frame(0, 1, f)), f)      # mirror twice
    assert same(api.orient_frame(2, 0, api.orient_frame(2, 0, f)), f)
    assert same(api.orient_frame(1, 0, api.orient_frame(1, 0, f)), api.orient_frame(2, 0, f))
    assert not same(api.orient_frame(2, 0, f), api.orient_frame(2, 1, f))
    for bad in ((4, 0), (-1, 0), (0, 2), (1, -1)):
        with pytest.raises(ValueError):
            api.orient_frame(*bad, f)


def test_abi_new_entry_points_and_nothing_else_moved():
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.ABI_SYMBOLS, name
    assert C.sizeof(api.DrvConfig) == 88 and api.DrvConfig._fields_[-1][0] == "quality_stats"
    lib.vp8hip_abi_version.restype = C.c_int
    assert lib.vp8hip_abi_version() == 4010 == api.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "vp8hip.h")).read() + open(os.path.join(ROOT, "include", "vp8hip_driver.h")).read() + \
        open(os.path.join(ROOT, "include", "vp8hip_host.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+VP8HIP_ABI_VERSION\s+4010\b", hdr)
    assert "source windows and orientation" in hdr
