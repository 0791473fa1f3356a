"""Segment data and contents for the normal loop filter's tests (test_lf_space_cpu.py says what they reach, test_gpu_lf_space.py runs
the device on them): every loop_filter_level, the sharpness values that take both shifts and the 9 - sharpness cap, both tables of
hev thresholds, on contents that put samples at the ends of the ranges inside which the kernels' rewritten edge arithmetic is exact."""
import numpy as np

from pipeline import default_segments

W = H = 144                     # 9 x 9 macroblocks: one past form 4's ring of 8 and one past the band of 8 rows
SHARPNESS = (0, 1, 4, 5, 7)     # none; >> 1; >> 1 with the cap 5 in force; >> 2; >> 2 with the cap 2
GEOMETRIES = [(1, 1), (1, 3), (3, 1), (1, 17), (17, 1), (9, 7), (9, 8), (9, 9), (7, 2), (8, 2), (9, 2), (15, 2), (16, 2), (17, 2), (33, 17)]
GEOMETRY_TABLES = [((6, 10, 14, 20), 0), ((15, 39, 40, 63), 0), ((15, 39, 40, 63), 7)]


def segments(levels, sharpness=0, key=False):
    """the 4 x 11 segment data fill_segment_data (vp8hip_dev.h; prepare_segments_data, vp8enc.cpp:129-221) leaves for these levels"""
    return default_segments(lf_levels=tuple(int(l) for l in levels), sharp=sharpness, inter=not key, key=key)


def sweep_parameters():
    """[(levels, sharpness, key)]: 160 tables.  Table k of a (key, sharpness) pair holds the levels k, k + 16, k + 32, k + 48 -- a low and
    a high one in every table -- rotated so that the lowest sits in segment (k + 3) % 4: level 0 in segment 3 (see SEEDS)."""
    return [(tuple(int(l) for l in np.roll([k, k + 16, k + 32, k + 48], (k + 3) % 4)), sharp, key)
            for key in (False, True) for sharp in SHARPNESS for k in range(16)]


def sweep():
    """[(tag, segment data)] of sweep_parameters()"""
    return [(f"{'key' if key else 'inter'} sharpness {sharp} levels {list(levels)}", segments(levels, sharp, key))
            for levels, sharp, key in sweep_parameters()]


def mb_mask(coeffs, parts):
    """prepare_filter_mask (loop_filter.h:25-55): inner edges are filtered in a split macroblock and in one with a coefficient; a whole
    macroblock's Y2 block counts, and the luma DCs it stands for do not"""
    c = np.abs(coeffs.astype(np.int64))
    n = c[:, :16, 1:].sum(axis=(1, 2)) + c[:, 16:24].sum(axis=(1, 2)) + np.where(parts == 0, c[:, 24].sum(axis=1), c[:, :16, 0].sum(axis=1))
    return np.where((parts != 0) | (n > 0), -1, 0).astype(np.int32)


def mb_inputs(mbs, rng):
    """coefficients, partitions and segment ids as test_gpu_simple_filter._inputs draws them, the Y2-DC-only macroblock included"""
    coeffs = np.zeros((mbs, 25, 16), np.int16)
    coeffs[rng.random(mbs) < 0.6, 3, 5] = 7
    coeffs[rng.random(mbs) < 0.2, 24, 0] = 3
    parts = (rng.random(mbs) < 0.3).astype(np.int32)
    seg = rng.integers(0, 4, size=mbs).astype(np.int32)
    return coeffs, parts, seg


# ---- contents -------------------------------------------------------------------------------------------------------------------
def _bounds_plane(h, w, rng):
    base = np.where(np.arange(h)[:, None] < h // 2, 0, 255)
    return np.clip(base + rng.integers(-40, 41, size=(h, w)) * (rng.random((h, w)) < 0.5), 0, 255).astype(np.uint8)


def bounds(w, h, rng, sd=None):
    """top half within 40 of 0, bottom half within 40 of 255: filtered samples leave 0..255, which only the store notices"""
    return _bounds_plane(h, w, rng), _bounds_plane(h // 2, w // 2, rng), _bounds_plane(h // 2, w // 2, rng)


def lf_check(w, h, rng, sd=None):
    """tests/lf_check.py's content: 8x8 squares with a little noise, some of it saturated"""
    base = rng.integers(0, 256, size=(h // 8 + 2, w // 8 + 2)).astype(np.float32)
    y = np.kron(base, np.ones((8, 8), np.float32))[:h, :w] + rng.integers(-6, 7, size=(h, w))
    y = np.clip(y * 1.3 - 30, 0, 255).astype(np.uint8)
    u = np.clip(np.kron(base[: h // 16 + 1, : w // 16 + 1], np.ones((8, 8), np.float32))[: h // 2, : w // 2] + rng.integers(-5, 6, size=(h // 2, w // 2)),
                0, 255).astype(np.uint8)
    return y, u, np.ascontiguousarray(u[::-1, ::-1])


def _clamp_profile(length, rng):
    """A line of `length` samples in cells of four.  Across the boundary between two cells the steps s3 = p0 - p1, s0 = q0 - p0 and
    s1 = q1 - q0 are drawn so that, for an interior limit near `it`,
      c1:    all three point the same way and add up to ~129..170: p1 - q1 passes +-128 while every interior difference stays <= it
             and 2|p0-q0| + |p1-q1|/2 stays under the edge limit of a level >= ~50;
      c2:    s0 points against s3 and s1: c128(p1 - q1) + 3 (q0 - p0) = +-(|s3| + |s1| + 2|s0|) passes +-127;
      short: the same with the sum drawn from 120..131, around the 124..127 the kernels' `123` covers.
    The sign is the one that keeps the line inside 0..255."""
    v = np.zeros(length + 4, np.int64)
    cur = int(rng.integers(60, 196))
    s3 = 0
    for c in range(0, length, 4):
        it = int(rng.choice([63, 60, 56, 50, 40, 30]))
        kind = rng.choice(["c1", "c2", "short", "calm"], p=[0.3, 0.3, 0.25, 0.15])
        if c == 0:
            s0 = s1 = 0
        elif kind == "c1":
            g = 1 if cur < 128 else -1
            m3, m1 = int(rng.integers(it - 12, it + 1)), int(rng.integers(it - 12, it + 1))
            s3, s1 = g * m3, g * m1
            s0 = g * max(3, 125 - m3 - m1 + int(rng.integers(0, 14)))
        elif kind in ("c2", "short"):
            g = -1 if cur < 128 else 1         # p0 = p1 - g |s3| moves towards the middle first
            if kind == "c2":
                m0 = int(rng.integers(it // 2, it))
                m3, m1 = int(rng.integers(it // 3, it * 4 // 5 + 1)), int(rng.integers(it // 3, it * 4 // 5 + 1))
            else:
                m0 = int(rng.integers(33, 44))
                rest = max(2, int(rng.integers(120, 132)) - 2 * m0)
                m3 = int(rng.integers(1, rest))
                m1 = rest - m3
            s3, s0, s1 = -g * m3, g * m0, -g * m1
        else:
            s3, s0, s1 = (int(x) for x in rng.integers(-3, 4, size=3))
        # the cell before this boundary ends p1, p0 = p1 + s3; this cell starts q0 = p0 + s0, q1 = q0 + s1, then a small step
        if c:
            v[c - 1] = v[c - 2] + s3
            cur = int(v[c - 1])
        a = cur + s0
        b = a + s1
        cc = b + int(rng.integers(-8, 9))
        v[c:c + 4] = (a, b, cc, cc)
        cur = cc
    return v[:length]


def _clamps_plane(h, w, rng, n):
    """the top 4/9 of the macroblock rows: every group of four pixel rows runs one profile along x (vertical edges meet it); the rest:
    every group of four pixel columns runs one along y (horizontal edges meet it); +-1 of noise on top"""
    split = max(1, (h // n) * 4 // 9) * n if h > n else 0
    p = np.zeros((h, w), np.int64)
    for y in range(0, split, 4):
        p[y:y + 4] = _clamp_profile(w, rng)[None, :]
    for x in range(0, w, 4):
        p[split:, x:x + 4] = _clamp_profile(h - split, rng)[:, None]
    return np.clip(p + rng.integers(-1, 2, size=(h, w)), 0, 255).astype(np.uint8)


def _with_bounds_stripe(p, rng, n):
    """the last two macroblock columns by bounds' recipe: the out-of-range carry inside this content too, behind macroblock and inner edges"""
    if p.shape[1] > 2 * n:
        p[:, -2 * n:] = _bounds_plane(p.shape[0], 2 * n, rng)
    return p


def clamps(w, h, rng, sd=None):
    return tuple(_with_bounds_stripe(p, rng, n) for p, n in zip(_clamps(w, h, rng), (16, 8, 8)))


def _clamps(w, h, rng):
    return _clamps_plane(h, w, rng, 16), _clamps_plane(h // 2, w // 2, rng, 8), _clamps_plane(h // 2, w // 2, rng, 8)


def _walk(n, targets, rng, period):
    """n block levels in 8..118; the step into block k is drawn around targets[0] where k is a multiple of `period` (a macroblock
    edge) and around targets[1] elsewhere (an inner edge), or is small"""
    out = np.zeros(n, np.int64)
    cur = int(rng.integers(8, 119))
    for k in range(n):
        if k:
            t = targets[0] if k % period == 0 else targets[1]
            s = int(rng.choice(t)) + int(rng.integers(-2, 3)) if rng.random() < 0.7 else int(rng.integers(0, 4))
            s = min(s, 110)
            s = s if rng.random() < 0.5 else -s
            if not 8 <= cur + s <= 118:
                s = -s
            if not 8 <= cur + s <= 118:
                s = 0
            cur += s
        out[k] = cur
    return out


def _limits_plane(h, w, rng, sd, n):
    """4x4 blocks, flat but for +-1: block (i, j) = fx[j] + fy[i], the steps of fx and fy drawn around 2/5 of an edge limit of the
    case (2|p0-q0| + |p1-q1|/2 of a step s between flat blocks is 2.5 s), so that the edge test lands on both sides of equality.  A
    third of the blocks carry a step inside -- along x or along y, in front of their second, third or fourth sample -- drawn around
    the case's interior limits and hev thresholds: those are tests of differences INSIDE a block."""
    sd = np.asarray(sd).reshape(4, 11)
    e_mb, e_b = [int(e) * 2 // 5 for e in sd[:, 7]], [int(e) * 2 // 5 for e in sd[:, 8]]
    inside = sorted(set(int(x) for x in sd[:, 9]) | set(int(x) for x in sd[:, 10]))
    by, bx = h // 4, w // 4
    fx, fy = _walk(bx, (e_mb, e_b), rng, n // 4), _walk(by, (e_mb, e_b), rng, n // 4)
    p = np.kron(fy[:, None] + fx[None, :], np.ones((4, 4), np.int64))
    d = (rng.choice(inside, size=(by, bx)) + rng.integers(-1, 3, size=(by, bx))) * rng.choice([-1, 1], size=(by, bx)) * (rng.random((by, bx)) < 0.33)
    k, along_x = rng.integers(1, 4, size=(by, bx)), rng.random((by, bx)) < 0.5
    up = lambda a: np.repeat(np.repeat(a, 4, axis=0), 4, axis=1)
    p += up(d * along_x) * ((np.arange(w) % 4)[None, :] >= up(k)) + up(d * ~along_x) * ((np.arange(h) % 4)[:, None] >= up(k))
    return np.clip(p + rng.integers(-1, 2, size=(h, w)), 0, 255).astype(np.uint8)


def limits(w, h, rng, sd):
    """the limits' blocks, with two macroblock columns of clamps' profiles (between flat blocks p1 - q1 is one step, at most 2/5 of an
    edge limit: the first clamp is out of reach) in front of two by bounds' recipe"""
    p = _limits_plane(h, w, rng, sd, 16), _limits_plane(h // 2, w // 2, rng, sd, 8), _limits_plane(h // 2, w // 2, rng, sd, 8)
    for q, n in zip(p, (16, 8, 8)):
        if q.shape[1] > 4 * n:
            q[:, -4 * n:-2 * n] = _clamps_plane(q.shape[0], 2 * n, rng, n)
    return tuple(_with_bounds_stripe(q, rng, n) for q, n in zip(p, (16, 8, 8)))


MAKERS = {"bounds": bounds, "limits": limits, "clamps": clamps, "lf_check": lf_check}
# One seed per content, for the macroblock data and the planes.  What they have to achieve is asserted in test_lf_space_cpu.py: the
# first macroblock of segment 3 comes behind macroblocks of segments 0, 1 and 2 (so the sweep's level-0 table filters with its three
# other levels before the plane ends), and the reach conditions of the content.
SEEDS = {"bounds": 1, "limits": 10, "clamps": 13, "lf_check": 18}


class Content:
    """one content at one size: macroblock data shared by all cases, planes per case where the content depends on the table"""

    def __init__(self, name, mbw=W // 16, mbh=H // 16, seed=None):
        self.name, self.W, self.H = name, mbw * 16, mbh * 16
        self.seed = SEEDS[name] if seed is None else seed
        rng = np.random.default_rng([self.seed, mbw, mbh])
        self.coeffs, self.parts, self.seg = mb_inputs(mbw * mbh, rng)
        self.mask = mb_mask(self.coeffs, self.parts)
        self.per_case = name == "limits"
        self._fixed = None if self.per_case else MAKERS[name](self.W, self.H, rng)

    def planes(self, sd=None, case=0):
        if not self.per_case:
            return self._fixed
        return limits(self.W, self.H, np.random.default_rng([self.seed, self.W, self.H, case]), sd)
