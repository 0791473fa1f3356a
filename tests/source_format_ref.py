"""The rule that makes 8-bit I420 of every source format (include/vp8hip_host.h), restated in numpy from its text, and makers of each
format's planes from arrays of sample values.  Shared by tests/test_source_format_cpu.py and tests/test_gpu_source_format.py.

Planes travel as flat uint8 arrays, the bytes a caller hands in: 16-bit samples are little-endian words."""
import numpy as np

I420, NV12, I422, I444, P010, I010, I210, I410 = range(8)
NAMES = ["I420", "NV12", "I422", "I444", "P010", "I010", "I210", "I410"]
ALL = list(range(8))
CONVERTED = ALL[1:]      # the seven formats that are not the default

# format -> (planes, chroma columns per output column, chroma rows per output row, depth)
_LAYOUT = {I420: (3, 1, 1, 8), NV12: (2, 1, 1, 8), I422: (3, 1, 2, 8), I444: (3, 2, 2, 8),
           P010: (2, 1, 1, 10), I010: (3, 1, 1, 10), I210: (3, 1, 2, 10), I410: (3, 2, 2, 10)}


def depth(fmt):
    return _LAYOUT[fmt][3]


def max_sample(fmt):
    return (1 << depth(fmt)) - 1


def chroma_shape(fmt, w, h):
    """(rows, columns) of one chroma component's samples as the format carries them"""
    _, nx, ny, _ = _LAYOUT[fmt]
    return (h // 2) * ny, (w // 2) * nx


def plane_bytes(fmt, w, h):
    planes, _, _, d = _LAYOUT[fmt]
    b = 2 if d > 8 else 1
    cr, cc = chroma_shape(fmt, w, h)
    return [w * h * b, cr * cc * b * (2 if planes == 2 else 1), cr * cc * b if planes == 3 else 0]


def make_planes(fmt, Y, U, V, junk=None):
    """sample arrays (values at the format's depth; U, V of chroma_shape) -> the format's planes as flat uint8 arrays.
    junk: an array of Y's shape (and any dtype) whose low six bits fill the bits of a 16-bit word that carry no value."""
    planes, _, _, d = _LAYOUT[fmt]

    def words(a, j):
        a = np.asarray(a).astype(np.uint16)
        if d == 8:
            return a.astype(np.uint8).ravel()
        j = np.zeros(a.shape, np.uint16) if j is None else (np.resize(np.asarray(j), a.shape).astype(np.uint16) & 63)
        w = ((a << 6) | j) if fmt == P010 else (a | (j << 10))
        return w.astype("<u2").ravel().view(np.uint8)

    if planes == 2:
        uv = np.stack([np.asarray(U), np.asarray(V)], axis=-1).reshape(np.asarray(U).shape[0], -1)
        return [words(Y, junk), words(uv, junk)]
    return [words(Y, junk), words(U, junk), words(V, junk)]


def samples(fmt, w, h, planes):
    """the format's planes -> (Y, U, V) arrays of sample values s (int32), chroma as the format carries it"""
    nplanes, _, _, d = _LAYOUT[fmt]

    def values(p):
        p = np.ascontiguousarray(p).ravel().view(np.uint8)
        if d == 8:
            return p.astype(np.int32)
        word = p.view("<u2").astype(np.int32)
        return word >> 6 if fmt == P010 else word & 1023

    cr, cc = chroma_shape(fmt, w, h)
    Y = values(planes[0]).reshape(h, w)
    if nplanes == 2:
        uv = values(planes[1]).reshape(cr, cc, 2)
        return Y, uv[:, :, 0], uv[:, :, 1]
    return Y, values(planes[1]).reshape(cr, cc), values(planes[2]).reshape(cr, cc)


def _round(S, k):
    return np.minimum(255, (S + (1 << (k - 1))) >> k if k else S).astype(np.uint8)


def convert_ref(fmt, w, h, planes):
    """the rule: out = min(255, (S + (1 << (k - 1))) >> k), S the sum of the n samples an output sample covers, k = log2(n) + d - 8"""
    _, nx, ny, d = _LAYOUT[fmt]
    Y, U, V = samples(fmt, w, h, planes)
    out = [_round(Y, d - 8)]
    k = {1: 0, 2: 1, 4: 2}[nx * ny] + d - 8
    for c in (U, V):
        S = c.reshape(h // 2, ny, w // 2, nx).sum(axis=(1, 3))
        out.append(_round(S, k))
    return tuple(out)


def random_samples(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    hi = max_sample(fmt) + 1
    return tuple(rng.integers(0, hi, s, dtype=np.int32) for s in ((h, w), chroma_shape(fmt, w, h), chroma_shape(fmt, w, h)))


def from_i420(fmt, y, u, v):
    """the format's planes that carry exactly this 8-bit I420 frame: chroma replicated, samples shifted up to the depth.  The rule
    returns the frame from them."""
    _, nx, ny, d = _LAYOUT[fmt]
    up = lambda a: np.asarray(a).astype(np.int32) << (d - 8)
    rep = lambda c: np.repeat(np.repeat(up(c), ny, axis=0), nx, axis=1)
    return make_planes(fmt, up(y), rep(u), rep(v))
