"""The two geometric stages of the input side (include/vp8hip_host.h: vp8hip_set_source_window, vp8hip_set_source_orientation)
restated in numpy, independently of the C++ and of the kernels, and the surfaces the tests feed them.  Shared by
tests/test_geometry_cpu.py, tests/test_gpu_geometry.py and tests/test_gpu_geometry_tools.py."""
import numpy as np

# format number -> per plane (horizontal shift, vertical shift, bytes per element); the table of include/vp8hip_host.h, typed again
I420, NV12, I422, I444, P010, I010, I210, I410, YUY2, UYVY, BGRA, RGBA = 0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19
TABLE = {
    I420: [(0, 0, 1), (1, 1, 1), (1, 1, 1)], NV12: [(0, 0, 1), (1, 1, 2)], I422: [(0, 0, 1), (1, 0, 1), (1, 0, 1)],
    I444: [(0, 0, 1), (0, 0, 1), (0, 0, 1)], P010: [(0, 0, 2), (1, 1, 4)], I010: [(0, 0, 2), (1, 1, 2), (1, 1, 2)],
    I210: [(0, 0, 2), (1, 0, 2), (1, 0, 2)], I410: [(0, 0, 2), (0, 0, 2), (0, 0, 2)],
    YUY2: [(1, 0, 4)], UYVY: [(1, 0, 4)], BGRA: [(0, 0, 4)], RGBA: [(0, 0, 4)],
}
ORIGINS = [(0, 0), (2, 6), (14, 2)]
EXTRA_PITCH = [0, 3, 64]
ORIENTATIONS = [(t, m) for t in range(4) for m in range(2)]


def tight_pitch(fmt, surface_width):
    """bytes of a row of each plane of a surface `surface_width` samples wide"""
    return [(surface_width >> hs) * bpe for hs, _, bpe in TABLE[fmt]]


def surface(fmt, surface_width, surface_height, pitch, rng):
    """random planes of a surface: plane p is a uint8 array of (rows, pitch[p])"""
    return [rng.integers(0, 256, (surface_height >> vs, pitch[p]), dtype=np.uint8) for p, (_, vs, _) in enumerate(TABLE[fmt])]


def window(fmt, planes, w, h, x, y):
    """the window's tight planes by numpy slicing: plane p is (h >> vs, (w >> hs) * bpe) bytes"""
    out = []
    for p, (hs, vs, bpe) in enumerate(TABLE[fmt]):
        out.append(np.ascontiguousarray(planes[p][y >> vs:(y >> vs) + (h >> vs), (x >> hs) * bpe:((x >> hs) + (w >> hs)) * bpe]))
    return out


def valid(fmt, w, h, x, y, pitch):
    if w <= 0 or h <= 0 or w & 1 or h & 1 or x < 0 or y < 0 or x & 1 or y & 1:
        return False
    return all(pitch[p] >= ((x + w) >> hs) * bpe for p, (hs, _, bpe) in enumerate(TABLE[fmt]))


def orient(frame, turns, mirror):
    """(Y, U, V) as they come in -> the upright planes: a left-right flip first, then `turns` clockwise quarter turns"""
    out = []
    for p in frame:
        s = np.asarray(p)[:, ::-1] if mirror else np.asarray(p)
        out.append(np.ascontiguousarray(np.rot90(s, -turns)))
    return out


def raw_frame(w, h, seed):
    """a random I420 frame of w x h with structure (a gradient under noise: a transposition or a flip never maps it onto itself)"""
    rng = np.random.default_rng(seed)
    out = []
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        g = (np.arange(ph)[:, None] * 3 + np.arange(pw)[None, :] * 5) & 127
        out.append((g + rng.integers(0, 128, (ph, pw))).astype(np.uint8))
    return out
