"""The overlay rule on the host (vp8host_overlay_frame; include/vp8hip_host.h, "OVERLAYS"): the plain C++ form against the numpy
restatement (tests/overlay_ref.py) byte for byte, the properties the header promises -- the two division identities exhaustively --
the identities (an opaque aligned layer is the BGRA rule, e = 0 changes nothing, two layers are two calls), every refusal, and the
stand-alone program that runs the rule under the address and undefined-behaviour sanitizers.  No GPU."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlay_ref as R
from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICTURES = [(40, 26), (34, 18), (2, 2)]
LAYERS = [(1, 1), (5, 3), (16, 16), (37, 21), (64, 40)]
ALPHAS = ["zero", "opaque", "random", "ramp"]
OPACITIES = [0, 1, 128, 254, 255]


def positions(pw, ph):
    return [(0, 0), (1, 1), (3, 2), (-3, -2), (pw - 5, ph - 3), (pw - 1, ph - 1), (pw, 0)]


def picture(pw, ph, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (ph, pw), dtype=np.uint8), rng.integers(0, 256, (ph // 2, pw // 2), dtype=np.uint8),
            rng.integers(0, 256, (ph // 2, pw // 2), dtype=np.uint8))


def layer(lw, lh, alpha, seed=2):
    rng = np.random.default_rng(seed + 100 * lw + lh)
    a = rng.integers(0, 256, (lh, lw, 4), dtype=np.uint8)
    if alpha == "zero":
        a[..., 3] = 0
    elif alpha == "opaque":
        a[..., 3] = 255
    elif alpha == "ramp":
        a[..., 3] = (np.arange(lw)[None, :] * 255 // max(lw - 1, 1) + np.arange(lh)[:, None]).clip(0, 255)
    return a


def same(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


# ---- the host function against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pic", PICTURES)
def test_host_function_equals_the_restatement(pic):
    pw, ph = pic
    src = picture(pw, ph)
    n = 0
    for (lw, lh), (x, y), alpha in itertools.product(LAYERS, positions(pw, ph), ALPHAS):
        opacity, matrix, fmt = OPACITIES[n % 5], (n // 5) % 4, (R.BGRA, R.RGBA)[(n // 20) % 2]      # (every value meets every layer, position and alpha kind)
        n += 1
        px = layer(lw, lh, alpha)
        got = api.overlay_frame(px, x, y, opacity, src, fmt, matrix)
        same(got, R.overlay_frame(px, x, y, opacity, src, fmt, matrix), (pic, lw, lh, x, y, alpha, opacity, matrix, fmt))
        if (x, y) == (pw, 0) or alpha == "zero" or opacity == 0:
            same(got, src, "outside the picture, or e = 0: nothing changes")


@pytest.mark.parametrize("fmt", [R.BGRA, R.RGBA])
@pytest.mark.parametrize("matrix", range(4))
def test_every_opacity_alpha_matrix_and_format(fmt, matrix):
    src = picture(40, 26, seed=5)
    for alpha, opacity in itertools.product(ALPHAS, OPACITIES):
        px = layer(37, 21, alpha, seed=7)
        same(api.overlay_frame(px, 3, 2, opacity, src, fmt, matrix), R.overlay_frame(px, 3, 2, opacity, src, fmt, matrix), (alpha, opacity))


def test_a_pitch_above_the_row_with_junk_between_the_rows():
    src = picture(40, 26)
    rng = np.random.default_rng(9)
    for lw, lh in LAYERS:
        wide = rng.integers(0, 256, (lh, lw + 3, 4), dtype=np.uint8)      # 12 junk bytes behind every row
        px = wide[:, :lw]
        assert px.strides[0] == 4 * (lw + 3)
        a = api.overlay_frame(px, 1, 1, 200, src)
        wide[:, lw:] ^= 0xff                                                # other junk, same layer
        b = api.overlay_frame(px, 1, 1, 200, src)
        same(a, b, "junk between the rows")
        same(a, R.overlay_frame(np.ascontiguousarray(px), 1, 1, 200, src), "pitched")


# ---- the properties the header lists -----------------------------------------------------------------------------------------------------
def test_the_two_division_identities_exhaustively():
    n = np.arange(0, 65026, dtype=np.int64)
    t = n + 128
    assert np.array_equal((n + 127) // 255, (t + (t >> 8)) >> 8)
    q = np.arange(0, 66299, dtype=np.int64)
    assert np.array_equal(q // 255, (q * 0x8081) >> 23)
    assert (66299 * 0x8081) >> 23 != 66299 // 255      # (the bound is the first q that fails)
    # the largest chroma q: src = 255 with E = 0, or every c_i at its largest with E = 1020
    for m in R.MATRICES.values():
        for row in m[2:]:
            c_max = sum(max(k, 0) for k in row) * 255 + 32768
            assert ((255 * 256 * 1020 + 130560) >> 10) <= 65408 and ((1020 * c_max + 130560) >> 10) <= 65408


@pytest.mark.parametrize("matrix", range(4))
def test_an_opaque_aligned_layer_is_the_bgra_rule(matrix):
    src = picture(40, 26)
    for (lw, lh), (x, y) in itertools.product([(16, 16), (6, 4), (2, 2)], [(0, 0), (2, 4), (24, 10)]):
        px = layer(lw, lh, "opaque")
        got = api.overlay_frame(px, x, y, 255, src, R.BGRA, matrix)
        ly, lu, lv = api.convert_frame(api.FORMAT_BGRA, lw, lh, [np.ascontiguousarray(px)], matrix)
        want = [p.copy() for p in src]
        want[0][y:y + lh, x:x + lw] = ly
        want[1][y // 2:(y + lh) // 2, x // 2:(x + lw) // 2] = lu
        want[2][y // 2:(y + lh) // 2, x // 2:(x + lw) // 2] = lv
        same(got, want, (lw, lh, x, y))


@pytest.mark.parametrize("matrix", range(4))
def test_chroma_range_over_the_rgb_cube(matrix):
    # the chroma of an opaque layer is affine in R, G, B per block: its extremes lie at the cube's corners; and every blend of two
    # values inside a range stays inside it (N is a weighted mean of src * 255 * 1024 / 1020-ths and the c_i)
    lo, hi = (16, 240) if matrix < 2 else (1, 255)
    src = (np.zeros((2, 2), np.uint8), np.full((1, 1), lo, np.uint8), np.full((1, 1), hi, np.uint8))
    seen = []
    for corner in itertools.product((0, 255), repeat=3):
        px = np.zeros((2, 2, 4), np.uint8)
        px[..., :3] = corner
        px[..., 3] = 255
        for opacity in (255, 128, 1):
            _, u, v = api.overlay_frame(px, 0, 0, opacity, src, R.BGRA, matrix)
            seen += [int(u[0, 0]), int(v[0, 0])]
    assert min(seen) >= lo and max(seen) <= hi, (min(seen), max(seen))
    grid = np.array(list(itertools.product(range(0, 256, 15), repeat=3)), np.uint8)      # 17^3 colours, one block each
    px = np.zeros((2, 2 * len(grid), 4), np.uint8)
    px[:, :, :3] = np.repeat(grid, 2, axis=0)[None]
    px[..., 3] = 255
    w = 2 * len(grid)
    _, u, v = api.overlay_frame(px, 0, 0, 255, (np.zeros((2, w), np.uint8), np.zeros((1, w // 2), np.uint8), np.zeros((1, w // 2), np.uint8)), R.BGRA, matrix)
    assert min(u.min(), v.min()) >= lo and max(u.max(), v.max()) <= hi


def test_two_layers_are_two_calls_in_slot_order():
    src = picture(40, 26)
    a, b = layer(16, 16, "random", seed=3), layer(37, 21, "ramp", seed=4)
    ab = api.overlay_frame(b, -3, -2, 254, api.overlay_frame(a, 3, 2, 128, src, R.BGRA, 1), R.RGBA, 2)
    ba = api.overlay_frame(a, 3, 2, 128, api.overlay_frame(b, -3, -2, 254, src, R.RGBA, 2), R.BGRA, 1)
    same(ab, R.overlay_layers([(a, 3, 2, 128, R.BGRA, 1), (b, -3, -2, 254, R.RGBA, 2)], src), "slot order")
    same(ba, R.overlay_layers([(b, -3, -2, 254, R.RGBA, 2), (a, 3, 2, 128, R.BGRA, 1)], src), "the other order")
    assert not all(np.array_equal(p, q) for p, q in zip(ab, ba))      # (the order matters)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = api.load_library()
    lib.vp8host_overlay_frame.argtypes = [C.c_int] * 5 + [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3
    px = np.zeros((3, 5, 4), np.uint8)
    y, u, v = (p.copy() for p in picture(40, 26))
    before = [p.copy() for p in (y, u, v)]
    good = dict(format=R.BGRA, matrix=0, lw=5, lh=3, pitch=20, pixels=px.ctypes.data, x=1, y=1, opacity=255, pw=40, ph=26, yp=y.ctypes.data,
                up=u.ctypes.data, vp=v.ctypes.data)
    call = lambda **kw: lib.vp8host_overlay_frame(*{**good, **kw}.values())
    assert call(opacity=0) == 0
    bad = [dict(format=0), dict(format=16), dict(format=17), dict(format=20), dict(format=-1), dict(matrix=-1), dict(matrix=4), dict(lw=0), dict(lh=0),
           dict(lw=-1), dict(lw=16385, pitch=4 * 16385), dict(lh=16385), dict(pitch=19), dict(pitch=0), dict(pitch=-20), dict(x=-16385), dict(x=16385),
           dict(y=-16385), dict(y=16385), dict(opacity=-1), dict(opacity=256), dict(pw=0), dict(ph=0), dict(pw=39), dict(ph=25), dict(pw=-2),
           dict(pixels=None), dict(yp=None), dict(up=None), dict(vp=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    same((y, u, v), before, "a refused call changes nothing")
    for kw in (dict(x=-16384, y=-16384), dict(x=16384, y=16384), dict(pitch=24)):
        assert call(**{**kw, "opacity": 0}) == 0, kw
    with pytest.raises(ValueError):
        api.overlay_frame(px, 0, 0, 256, before)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_host_rule_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "overlay_sanitize")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "native", "overlay_sanitize.cpp"), os.path.join(ROOT, "vp8oclenc_amd", "csrc", "vp8_host.cpp"),
                    "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("clean"), r.stdout + r.stderr
