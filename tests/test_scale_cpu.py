"""The scaler's arithmetic contract without a GPU: a numpy restatement of include/vp8hip_host.h's vp8host_scale_taps and of the two
passes k_scale_b runs (tests/test_gpu_scale.py holds the kernel to it bit for bit), the host tables against it, the identities the
contract promises, and the grown vp8drv_config against its Python mirror."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREA, LANCZOS = 0, 1
MAX_TAPS = 32
SIZES = [(3840, 1920), (1920, 1280), (1080, 720), (1920, 640), (640, 128), (1278, 714), (1280, 1278), (65, 33), (49, 17), (64, 64)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _lanczos3(x: float) -> float:
    if abs(x) >= 3.0:
        return 0.0
    if x == 0.0:
        return 1.0
    a, b = math.pi * x, math.pi * x / 3.0
    return (math.sin(a) / a) * (math.sin(b) / b)


def _span(i, n_in, n_out, kind):
    if kind == AREA:
        return i * n_in // n_out, ((i + 1) * n_in - 1) // n_out
    r = n_in / n_out
    c = (i + 0.5) * r - 0.5
    return math.ceil(c - 3.0 * r), math.floor(c + 3.0 * r)


def ref_taps(n_in: int, n_out: int, kind: int):
    """-> (n, start [n_out], coef [n_out, n]) by the formulas of the contract, or None where the contract refuses the pair"""
    if not (1 <= n_out <= n_in <= 16384):
        return None
    spans = [_span(i, n_in, n_out, kind) for i in range(n_out)]
    n = max(b - a + 1 for a, b in spans)
    if n > MAX_TAPS or n > n_in:
        return None
    start = np.zeros(n_out, np.int32)
    coef = np.zeros((n_out, n), np.int64)
    for i, (a, b) in enumerate(spans):
        if kind == AREA:
            # cum_j: of output i's interval [i n_in, (i + 1) n_in), the length left of sample j's right end (j + 1) n_out
            cum = [min(max((j + 1) * n_out - i * n_in, 0), n_in) for j in range(a - 1, b + 1)]
            w = [4096 * cum[k + 1] // n_in - 4096 * cum[k] // n_in for k in range(b - a + 1)]
        else:
            r = n_in / n_out
            c = (i + 0.5) * r - 0.5
            f = [_lanczos3((j - c) / r) for j in range(a, b + 1)]
            total = 0.0
            for v in f:
                total += v
            w = [math.floor(4096.0 * v / total + 0.5) for v in f]
        s = min(max(a, 0), n_in - n)      # taps outside the plane fold onto the edge sample
        for k, v in enumerate(w):
            coef[i, min(max(a + k, 0), n_in - 1) - s] += v
        if kind == LANCZOS:
            coef[i, int(np.argmax(coef[i]))] += 4096 - int(coef[i].sum())
        start[i] = s
    if np.abs(coef).sum(axis=1).max() > 8000:
        return None
    return n, start, coef.astype(np.int16)


def ref_scale_plane(src: np.ndarray, start_x, cx, start_y, cy) -> np.ndarray:
    """The two passes in int32: horizontal into an intermediate that must stay inside int16, vertical out of it, clamped"""
    src = src.astype(np.int32)
    h_in, w_in = src.shape
    nx, ny = cx.shape[1], cy.shape[1]
    assert start_x.min() >= 0 and (start_x + nx).max() <= w_in and start_y.min() >= 0 and (start_y + ny).max() <= h_in
    t = np.full((h_in, len(start_x)), 32, np.int32)
    for k in range(nx):
        t += cx[:, k].astype(np.int32)[None, :] * src[:, start_x + k]
    t >>= 6
    assert t.min() >= -32768 and t.max() <= 32767, "the intermediate leaves int16"
    out = np.full((len(start_y), len(start_x)), 1 << 17, np.int32)
    for k in range(ny):
        out += cy[:, k].astype(np.int32)[:, None] * t[start_y + k, :]
    return np.clip(out >> 18, 0, 255).astype(np.uint8)


def ref_scale_plane_by_tables(src, w_out, h_out, kind, taps=ref_taps):
    h_in, w_in = src.shape
    _, sx, cx = taps(w_in, w_out, kind)
    _, sy, cy = taps(h_in, h_out, kind)
    return ref_scale_plane(src, sx, cx, sy, cy)


def ref_scale_frame(y, u, v, dst_w, dst_h, kind, taps=ref_taps):
    """I420 planes of any even size -> the planes of dst_w x dst_h, every plane on its own (chroma: in / 2 -> dst / 2)"""
    return (ref_scale_plane_by_tables(y, dst_w, dst_h, kind, taps), ref_scale_plane_by_tables(u, dst_w // 2, dst_h // 2, kind, taps),
            ref_scale_plane_by_tables(v, dst_w // 2, dst_h // 2, kind, taps))


def pad_plane(p, w, h):
    """copy_with_padding: the last sample of a row to the right, the last row downwards"""
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def lib_taps(n_in, n_out, kind):
    try:
        return api.scale_taps(n_in, n_out, kind)
    except ValueError:
        return None


# ---- 1. the host tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", SIZES + [(2160, 360)])
def test_area_tables_equal_the_restatement(n_in, n_out):
    got, want = lib_taps(n_in, n_out, AREA), ref_taps(n_in, n_out, AREA)
    assert got is not None and want is not None
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert (got[2].astype(np.int64).sum(axis=1) == 4096).all()
    assert got[1].min() >= 0 and (got[1] + got[0]).max() <= n_in


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_lanczos_tables_equal_the_restatement_within_one(n_in, n_out):
    got, want = lib_taps(n_in, n_out, LANCZOS), ref_taps(n_in, n_out, LANCZOS)
    assert got is not None and want is not None
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    assert (got[2].astype(np.int64).sum(axis=1) == 4096).all() and (want[2].astype(np.int64).sum(axis=1) == 4096).all()
    assert np.abs(got[2].astype(np.int32) - want[2].astype(np.int32)).max() <= 1
    assert np.abs(got[2].astype(np.int32)).sum(axis=1).max() <= 8000
    assert got[1].min() >= 0 and (got[1] + got[0]).max() <= n_in


def test_tap_counts_and_refusals():
    assert lib_taps(2160, 360, AREA)[0] == 6
    assert lib_taps(2160, 360, LANCZOS) is None and ref_taps(2160, 360, LANCZOS) is None      # 36 taps
    for kind in (AREA, LANCZOS):
        assert lib_taps(66, 2, kind) is None and ref_taps(66, 2, kind) is None                # 33 and more
        assert lib_taps(64, 65, kind) is None          # no upscaling
        assert lib_taps(16386, 8192, kind) is None
    assert lib_taps(64, 32, 2) is None
    counts = {kind: [lib_taps(a, b, kind)[0] for a, b in SIZES] for kind in (AREA, LANCZOS)}
    assert min(counts[AREA]) == 1 and max(counts[AREA]) <= 8
    assert min(counts[LANCZOS]) == 7 and max(counts[LANCZOS]) == 31


# ---- 2. identities -------------------------------------------------------------------------------------------------------------------
def test_area_at_two_to_one_is_the_pyramid_filter():
    rng = np.random.default_rng(5)
    for w, h in ((64, 48), (130, 98), (3840, 16)):
        src = rng.integers(0, 256, (h, w), dtype=np.uint8)
        s = src.astype(np.int32)
        want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
        for taps in (ref_taps, lib_taps):
            assert np.array_equal(ref_scale_plane_by_tables(src, w // 2, h // 2, AREA, taps), want)


@pytest.mark.parametrize("kind", [AREA, LANCZOS])
def test_a_constant_plane_stays_constant_and_equal_sizes_are_the_identity(kind):
    rng = np.random.default_rng(6)
    for n_in, n_out in SIZES:
        n, start, coef = lib_taps(n_in, n_out, kind)
        for value in (0, 1, 127, 254, 255):
            rows = np.full((3, n_in), value, np.uint8)
            cols = np.full((n_in, 3), value, np.uint8)
            ident = (1, np.arange(3, dtype=np.int32), np.full((3, 1), 4096, np.int16))
            assert (ref_scale_plane(rows, start, coef, ident[1], ident[2]) == value).all()
            assert (ref_scale_plane(cols, ident[1], ident[2], start, coef) == value).all()
    src = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    assert np.array_equal(ref_scale_plane_by_tables(src, 64, 64, kind, lib_taps), src)


def test_extreme_planes_keep_the_intermediate_inside_int16():
    """an all-0 / all-255 checkerboard and stripes through the Lanczos tables with the largest sum of |c|: the assertion inside
    ref_scale_plane is the check"""
    n_in, n_out = 1280, 1278
    yy, xx = np.mgrid[0:16, 0:n_in]
    for src in (((yy + xx) & 1) * 255, (xx & 1) * 255, ((xx >> 1) & 1) * 255):
        out = ref_scale_plane_by_tables(src.astype(np.uint8), n_out, 16, LANCZOS, lib_taps)
        assert out.shape == (16, n_out)


# ---- 3. the grown configuration ----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_driver_config_grew_by_three_ints_and_the_mirror_agrees(tmp_path):
    src = tmp_path / "c.c"
    src.write_text("""
        #include <stdio.h>
        #include <stddef.h>
        #include "vp8hip_driver.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(vp8drv_config), offsetof(vp8drv_config, loop_filter_type), offsetof(vp8drv_config, in_width),
                   offsetof(vp8drv_config, in_height), offsetof(vp8drv_config, scale_filter), offsetof(vp8drv_config, quality_stats));
            return 0;
        }""")
    exe = tmp_path / "c"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = api.DrvConfig
    assert c == [C.sizeof(D), D.loop_filter_type.offset, D.in_width.offset, D.in_height.offset, D.scale_filter.offset, D.quality_stats.offset]
    # three int32 more than the nineteen fields before them; they stand between loop_filter_type and quality_stats, which stays last
    assert c[0] == 22 * 4 and c[2:] == [c[1] + 4, c[1] + 8, c[1] + 12, c[1] + 16] and c[5] == c[0] - 4
    lib = api.load_library()
    cfg = D()
    cfg.in_width = cfg.in_height = cfg.scale_filter = 7
    lib.vp8drv_default_config.argtypes = [C.POINTER(D)]
    lib.vp8drv_default_config.restype = None
    lib.vp8drv_default_config(C.byref(cfg))
    assert (cfg.in_width, cfg.in_height, cfg.scale_filter) == (0, 0, 0)
    for name in ("vp8hip_set_source_scaling", "vp8host_scale_taps"):
        assert hasattr(lib, name), name
