"""The rule of the packed source formats -- YUY2, UYVY, BGRA, RGBA and the colour matrix of the RGB pair -- restated in numpy from the
text of include/vp8hip_host.h (not from the C++), makers of frames, and the floating-point BT.601 / BT.709 definitions the integer
tables approximate.  Shared by tests/test_packed_format_cpu.py and tests/test_gpu_packed_format.py.

A frame is ONE flat uint8 array: the bytes a caller hands in."""
import numpy as np

YUY2, UYVY, BGRA, RGBA = 16, 17, 18, 19
NAMES = {YUY2: "YUY2", UYVY: "UYVY", BGRA: "BGRA", RGBA: "RGBA"}
PACKED = [YUY2, UYVY, BGRA, RGBA]
RGB = (BGRA, RGBA)
BT601_LIMITED, BT709_LIMITED, BT601_FULL, BT709_FULL = range(4)
MATRICES = [0, 1, 2, 3]

# the header's table: m -> (off, Y row, U row, V row), each row R, G, B, times 256
TABLE = {
    0: (16, (66, 129, 25), (-38, -74, 112), (112, -94, -18)),
    1: (16, (47, 157, 16), (-26, -86, 112), (112, -102, -10)),
    2: (0, (77, 150, 29), (-43, -84, 127), (127, -106, -21)),
    3: (0, (54, 183, 19), (-29, -98, 127), (127, -116, -11)),
}


def plane_bytes(fmt, w, h):
    return [(4 if fmt in RGB else 2) * w * h, 0, 0]


def _rgb(fmt, w, h, frame):
    """(R, G, B) int64 arrays of h x w"""
    p = np.ascontiguousarray(frame).ravel().view(np.uint8).reshape(h, w, 4).astype(np.int64)
    return (p[:, :, 2], p[:, :, 1], p[:, :, 0]) if fmt == BGRA else (p[:, :, 0], p[:, :, 1], p[:, :, 2])


def convert_ref(fmt, w, h, frame, matrix=0):
    """the rule -> (Y, U, V) uint8"""
    if fmt in (YUY2, UYVY):
        p = np.ascontiguousarray(frame).ravel().view(np.uint8).reshape(h, w // 2, 4).astype(np.int64)
        y0, u, y1, v = (p[:, :, i] for i in ((0, 1, 2, 3) if fmt == YUY2 else (1, 0, 3, 2)))
        Y = np.empty((h, w), np.int64)
        Y[:, 0::2], Y[:, 1::2] = y0, y1
        return (Y.astype(np.uint8),) + tuple(((c[0::2] + c[1::2] + 1) >> 1).astype(np.uint8) for c in (u, v))
    off, cy, cu, cv = TABLE[matrix]
    R, G, B = _rgb(fmt, w, h, frame)
    dot = lambda c: c[0] * R + c[1] * G + c[2] * B
    Y = off + ((dot(cy) + 128) >> 8)
    out = [Y]
    for c in (cu, cv):
        S = dot(c).reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3))
        assert (S + 131584).min() >= 0
        out.append((S + 131072 + 512) >> 10)
    for o in out:
        assert 0 <= o.min() and o.max() <= 255      # "no clamp is needed"
    return tuple(o.astype(np.uint8) for o in out)


def float_ref(matrix, R, G, B):
    """the BT.601 / BT.709 definitions in floating point on arrays of 8-bit R, G, B -> (Y, Cb, Cr), not rounded"""
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[matrix & 1]
    kg = 1.0 - kr - kb
    r, g, b = (np.asarray(c, np.float64) / 255.0 for c in (R, G, B))
    y = kr * r + kg * g + kb * b
    pb, pr = 0.5 * (b - y) / (1.0 - kb), 0.5 * (r - y) / (1.0 - kr)
    if matrix < 2:
        return 16.0 + 219.0 * y, 128.0 + 224.0 * pb, 128.0 + 224.0 * pr
    return 255.0 * y, 128.0 + 255.0 * pb, 128.0 + 255.0 * pr


# ---- makers of frames -------------------------------------------------------------------------------------------------------------------
def make_rgb(fmt, R, G, B, A=None):
    R, G, B = (np.asarray(c).astype(np.uint8) for c in (R, G, B))
    A = np.full(R.shape, 255, np.uint8) if A is None else np.resize(np.asarray(A), R.shape).astype(np.uint8)
    return np.ascontiguousarray(np.stack((B, G, R, A) if fmt == BGRA else (R, G, B, A), axis=-1)).ravel()


def make_422(fmt, Y, U, V):
    """Y of h x w, U and V of h x w/2 (the I422 frame's samples) -> the packed frame"""
    Y, U, V = (np.asarray(c).astype(np.uint8) for c in (Y, U, V))
    q = np.empty((Y.shape[0], Y.shape[1] // 2, 4), np.uint8)
    ly, lu = (0, 1) if fmt == YUY2 else (1, 0)
    q[:, :, ly], q[:, :, ly + 2], q[:, :, lu], q[:, :, lu + 2] = Y[:, 0::2], Y[:, 1::2], U, V
    return q.ravel()


def from_i420(fmt, y, u, v):
    """the YUY2 / UYVY frame that carries exactly this I420 frame: chroma rows replicated"""
    assert fmt in (YUY2, UYVY)
    return make_422(fmt, y, np.repeat(np.asarray(u), 2, axis=0), np.repeat(np.asarray(v), 2, axis=0))


def rgb_near_i420(fmt, y, u, v):
    """an RGB frame (alpha 255) that looks like this I420 frame: the float inverse of BT.601 limited range, chroma replicated,
    clipped.  Not exact: a picture for the end-to-end tests, whose expected bytes come from the rule applied to IT"""
    Y = np.asarray(y, np.float32) - 16.0
    U, V = (np.repeat(np.repeat(np.asarray(p, np.float32) - 128.0, 2, axis=0), 2, axis=1) for p in (u, v))
    clip = lambda c: np.clip(np.rint(c), 0, 255)
    return make_rgb(fmt, clip(1.164 * Y + 1.596 * V), clip(1.164 * Y - 0.392 * U - 0.813 * V), clip(1.164 * Y + 2.017 * U))


def grey_rgb(fmt, y):
    """R = G = B = y: at the full matrices the rule gives (y, 128, 128)"""
    return make_rgb(fmt, y, y, y)


CORNERS = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)


def corner_frame(fmt, w, h):
    """the eight corners of the RGB cube: the top half in 2x2-uniform blocks, the bottom half pixel by pixel (2x2-mixed blocks)"""
    idx = np.empty((h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    idx[:] = (yy // 2 * 3 + xx // 2) % 8
    mixed = (yy * 5 + xx * 3 + (yy * xx) % 7) % 8
    idx[h // 2:] = mixed[h // 2:]
    c = CORNERS[idx]
    return make_rgb(fmt, c[:, :, 0], c[:, :, 1], c[:, :, 2], A=(yy * 31 + xx * 17) & 255)


def frames_for(fmt, w, h):
    """random with junk alpha, all 255, all 0, and (RGB) the cube corners / (4:2:2) a second random frame"""
    rng = np.random.default_rng(1000 + fmt)
    if fmt in RGB:
        rnd = lambda: rng.integers(0, 256, (h, w))
        return [make_rgb(fmt, rnd(), rnd(), rnd(), A=rnd()), np.full(4 * w * h, 255, np.uint8), np.zeros(4 * w * h, np.uint8), corner_frame(fmt, w, h)]
    return [rng.integers(0, 256, 2 * w * h).astype(np.uint8), np.full(2 * w * h, 255, np.uint8), np.zeros(2 * w * h, np.uint8),
            rng.integers(0, 256, 2 * w * h).astype(np.uint8)]
