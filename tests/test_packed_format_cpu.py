"""The packed source formats on the host (no GPU): vp8host_convert_frame_colour against the numpy restatement of the header's rule
(tests/packed_format_ref.py) bit for bit, the properties the header claims for its tables, the refusals, and the stand-alone program that
runs the host rule under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import packed_format_ref as P
import source_format_ref as R
from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(34, 18), (16, 16), (10, 6), (2, 2), (200, 120)]


def same(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fmt", P.PACKED)
def test_the_host_rule_equals_the_restatement_bit_for_bit(fmt, size):
    w, h = size
    for i, frame in enumerate(P.frames_for(fmt, w, h)):
        for m in P.MATRICES:
            same(api.convert_frame(fmt, w, h, [frame], matrix=m), P.convert_ref(fmt, w, h, frame, m), (P.NAMES[fmt], size, i, m))
        same(api.convert_frame(fmt, w, h, [frame]), P.convert_ref(fmt, w, h, frame, 0), (P.NAMES[fmt], size, i, "no matrix"))


def test_the_library_has_the_headers_tables():
    for m in P.MATRICES:
        c, off = api.colour_coefficients(m)
        assert off == P.TABLE[m][0] and c.tolist() == [list(r) for r in P.TABLE[m][1:]]
    header = open(os.path.join(ROOT, "include", "vp8hip_host.h")).read()
    for m, (off, *rows) in P.TABLE.items():      # ... and the header's text has the restatement's
        nums = r"\s+".join(str(x) for x in [off] + [c for r in rows for c in r])
        import re
        assert re.search(rf"\*\s+{m} BT\d+_\w+\s+{nums}\b", header), m


def test_the_properties_the_header_claims():
    cube = P.CORNERS.astype(np.int64)
    for m, (off, cy, cu, cv) in P.TABLE.items():
        full = m >= 2
        assert sum(cy) == (256 if full else 220)
        assert sum(cu) == 0 and sum(cv) == 0
        assert all(0 <= c <= 255 for c in cy) and all(-128 <= c <= 127 for c in cu + cv)
        assert off == (0 if full else 16)
        # grey gives exactly 128, and Y = v at the full matrices: every v, as 2x2 frames through the rule
        for fmt in P.RGB:
            v = np.arange(256)
            frame = P.make_rgb(fmt, *[np.repeat(np.repeat(v[None, :], 2, axis=0), 2, axis=1)] * 3, A=np.arange(1024) * 7)
            y, u, vv = P.convert_ref(fmt, 512, 2, frame, m)
            assert (u == 128).all() and (vv == 128).all()
            if full:
                assert (y == np.repeat(v, 2)[None, :]).all()
            else:
                assert y.min() == 16 and y.max() == 235
        # ranges over the cube corners: per pixel for luma, over all-equal 2x2 blocks for chroma
        R_, G_, B_ = cube[:, 0], cube[:, 1], cube[:, 2]
        Y = off + ((cy[0] * R_ + cy[1] * G_ + cy[2] * B_ + 128) >> 8)
        assert (Y.min(), Y.max()) == ((0, 255) if full else (16, 235))
        for c in (cu, cv):
            S = 4 * (c[0] * R_ + c[1] * G_ + c[2] * B_)
            assert (S + 131584).min() >= 0
            o = (S + 131072 + 512) >> 10
            lo, hi = (1, 255) if full else (16, 240)
            assert lo <= o.min() and o.max() <= hi, (m, o.min(), o.max())
            assert o.min() == lo and o.max() == hi
        # (the extremes of a linear form over the cube are at its corners; mixed 2x2 blocks lie between the uniform ones)
        frame = P.corner_frame(P.BGRA, 16, 16)
        y, u, vv = P.convert_ref(P.BGRA, 16, 16, frame, m)
        assert (0 if full else 16) <= y.min() and y.max() <= (255 if full else 235)
        assert min(u.min(), vv.min()) >= (1 if full else 16) and max(u.max(), vv.max()) <= (255 if full else 240)


def test_the_distance_from_the_float_definition_is_at_most_2():
    """100 000 seeded pixels, each its own all-equal 2x2 block.  The margin: 1.62 measured at the full matrices (0.5 is carried as
    127 / 256), 1.12 at the limited ones, rounded up to the next integer."""
    rng = np.random.default_rng(2024)
    n = 100000
    rgb = rng.integers(0, 256, (n, 3))
    px = np.repeat(np.repeat(rgb[None, :, :], 2, axis=0), 2, axis=1)      # 2 rows x 2n pixels
    frame = P.make_rgb(P.RGBA, px[:, :, 0], px[:, :, 1], px[:, :, 2])
    for m in P.MATRICES:
        y, u, v = api.convert_frame(P.RGBA, 2 * n, 2, [frame], matrix=m)
        fy, fu, fv = P.float_ref(m, rgb[:, 0], rgb[:, 1], rgb[:, 2])
        d = max(np.abs(y[0, 0::2] - fy).max(), np.abs(u[0] - fu).max(), np.abs(v[0] - fv).max())
        print(f"matrix {m}: largest distance from the float definition {d:.3f}")
        assert d <= 2.0, (m, d)


@pytest.mark.parametrize("fmt", [P.YUY2, P.UYVY])
def test_packed_422_converts_to_what_the_i422_frame_of_the_same_samples_converts_to(fmt):
    for w, h in SIZES:
        Y, U, V = R.random_samples(R.I422, w, h, 50 + fmt)
        got = api.convert_frame(fmt, w, h, [P.make_422(fmt, Y, U, V)])
        same(got, api.convert_frame(R.I422, w, h, R.make_planes(R.I422, Y, U, V)), (P.NAMES[fmt], w, h))
        same(got, R.convert_ref(R.I422, w, h, R.make_planes(R.I422, Y, U, V)), (P.NAMES[fmt], w, h, "ref"))
    # ... and a frame made from I420 gives the I420 frame back
    y, u, v = (np.random.default_rng(3).integers(0, 256, s, dtype=np.uint8) for s in ((18, 34), (9, 17), (9, 17)))
    same(api.convert_frame(fmt, 34, 18, [P.from_i420(fmt, y, u, v)]), (y, u, v), "from_i420")
    same(api.convert_frame(fmt, 34, 18, api.planes_from_i420(fmt, y, u, v)), (y, u, v), "api.planes_from_i420")


@pytest.mark.parametrize("fmt", P.RGB)
def test_alpha_changes_nothing(fmt):
    rng = np.random.default_rng(5)
    w, h = 34, 18
    c = [rng.integers(0, 256, (h, w)) for _ in range(3)]
    for m in P.MATRICES:
        want = api.convert_frame(fmt, w, h, [P.make_rgb(fmt, *c, A=np.zeros((h, w)))], matrix=m)
        for k in range(3):
            same(api.convert_frame(fmt, w, h, [P.make_rgb(fmt, *c, A=rng.integers(0, 256, (h, w)))], matrix=m), want, (fmt, m, k))


def test_plane_bytes_names_and_refusals():
    lib = api.load_library()
    lib.vp8host_source_plane_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    b = (C.c_size_t * 3)()
    for w, h in SIZES + [(1920, 1080), (16384, 16384)]:
        for fmt in P.PACKED:
            assert lib.vp8host_source_plane_bytes(fmt, w, h, b) == 0
            assert list(b) == P.plane_bytes(fmt, w, h) == api.source_plane_bytes(fmt, w, h)
    for fmt in list(range(8, 16)) + [20, 21, -1, 1 << 20]:
        assert lib.vp8host_source_plane_bytes(fmt, 16, 16, b) == -1, fmt
        with pytest.raises(ValueError):
            api.source_format(fmt)
    for fmt in P.PACKED:
        for w, h in ((17, 16), (16, 15), (0, 16), (16, -2)):
            assert lib.vp8host_source_plane_bytes(fmt, w, h, b) == -1
        assert lib.vp8host_source_plane_bytes(fmt, 16, 16, None) == -1
    assert [api.source_format(n) for n in ("yuy2", "UYVY", "bgra", "Rgba")] == P.PACKED
    assert [api.source_format(n) for n in P.PACKED] == P.PACKED
    assert [api.source_colour(a, b_) for b_ in ("limited", "full") for a in ("bt601", "bt709")] == [0, 1, 2, 3]
    assert api.source_colour("BT709", "Full") == P.BT709_FULL and api.source_colour(2) == 2
    for bad in (("bt2020", "limited"), ("bt601", "wide"), (4, "limited"), (-1, "limited")):
        with pytest.raises(ValueError):
            api.source_colour(*bad)
    lib.vp8host_convert_frame.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6
    lib.vp8host_convert_frame_colour.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6
    lib.vp8host_colour_coefficients.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    buf = np.zeros(8192, np.uint8)
    p = buf.ctypes.data
    out = (p + 4096, p + 5120, p + 6144)
    assert lib.vp8host_convert_frame(8, 16, 16, p, p, p, *out) == -1      # still
    for fmt in list(range(8, 16)) + [20]:
        assert lib.vp8host_convert_frame(fmt, 16, 16, p, p, p, *out) == -1
        assert lib.vp8host_convert_frame_colour(fmt, 0, 16, 16, p, p, p, *out) == -1
    for fmt in P.PACKED:
        assert lib.vp8host_convert_frame_colour(fmt, 0, 16, 16, p, None, None, *out) == 0      # one plane: the others are not read
        assert lib.vp8host_convert_frame(fmt, 16, 16, p, None, None, *out) == 0
        for m in (4, -1):
            assert lib.vp8host_convert_frame_colour(fmt, m, 16, 16, p, p, p, *out) == -1
        for w, h in ((15, 16), (16, 17), (0, 0)):
            assert lib.vp8host_convert_frame_colour(fmt, 0, w, h, p, p, p, *out) == -1
        assert lib.vp8host_convert_frame_colour(fmt, 0, 16, 16, None, p, p, *out) == -1
        for k in range(3):
            o = list(out)
            o[k] = None
            assert lib.vp8host_convert_frame_colour(fmt, 0, 16, 16, p, p, p, *o) == -1
    assert lib.vp8host_convert_frame_colour(R.NV12, 4, 16, 16, p, p, p, *out) == -1      # the matrix is checked for every format
    assert lib.vp8host_convert_frame_colour(R.NV12, 3, 16, 16, p, p + 256, None, *out) == 0
    c9 = (C.c_int32 * 9)()
    off = C.c_int32()
    for m in (4, -1):
        assert lib.vp8host_colour_coefficients(m, c9, C.byref(off)) == -1
    assert lib.vp8host_colour_coefficients(0, None, C.byref(off)) == -1 and lib.vp8host_colour_coefficients(0, c9, None) == -1
    for name in ("vp8hip_set_source_colour", "vp8drv_set_source_colour", "vp8host_convert_frame_colour", "vp8host_colour_coefficients"):
        assert name in api.ABI_SYMBOLS and hasattr(lib, name), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_host_rule_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "convert_packed_sanitize")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "native", "convert_packed_sanitize.cpp"), os.path.join(ROOT, "vp8oclenc_amd", "csrc", "vp8_host.cpp"),
                    "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("clean"), r.stdout + r.stderr
