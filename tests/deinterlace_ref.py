"""The deinterlacer's rule (include/vp8hip_host.h, vp8hip_set_deinterlace) restated in numpy, independently of the C++ and of the
kernel, and the input sequences the tests feed it.  Shared by tests/test_deinterlace_cpu.py, tests/test_gpu_deinterlace.py and
tests/test_gpu_deinterlace_tools.py."""
import numpy as np


def spatial(plane, keep):
    """the spatial value s of EVERY row of a plane (the rule only uses it on missing rows), int32"""
    p = np.asarray(plane).astype(np.int32)
    h = p.shape[0]
    K = p[keep::2]
    n = K.shape[0]
    y = np.arange(h)
    j0 = (y - 1 - keep) // 2      # floor division: -1 for y = 0, keep = 1
    a = [K[np.clip(j0 + k, 0, n - 1)] for k in (-1, 0, 1, 2)]
    return np.clip((-a[0] + 9 * a[1] + 9 * a[2] - a[3] + 8) >> 4, 0, 255)


def deinterlace_plane(cur, hist, keep):
    """one plane -> (out uint8, woven mask of the missing rows' samples); hist None: no history"""
    cur = np.asarray(cur, np.uint8)
    h = cur.shape[0]
    missing = (np.arange(h) & 1) != keep
    s = spatial(cur, keep)
    out = cur.astype(np.int32).copy()
    if hist is None:
        out[missing] = s[missing]
        woven = np.zeros(cur.shape, bool)
    else:
        d = np.abs(cur.astype(np.int32) - np.asarray(hist).astype(np.int32))
        y = np.arange(h)
        m = np.maximum(d, np.maximum(d[np.maximum(y - 1, 0)], d[np.minimum(y + 1, h - 1)]))
        wv = cur.astype(np.int32)
        o = np.minimum(np.maximum(s, wv - m), wv + m)
        out[missing] = o[missing]
        woven = (o == wv) & missing[:, None]
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8), woven


class Deinterlacer:
    """a context's deinterlacer: mode (0 off, 1 field, 2 adaptive), keep (0 top, 1 bottom), the history, restart;
    take(frame) -> (planes, woven, missing)"""

    def __init__(self, mode, keep):
        self.mode, self.keep = mode, keep
        self.hist = None

    def restart(self):
        self.hist = None

    def take(self, frame):
        frame = [np.ascontiguousarray(p, np.uint8) for p in frame]
        if not self.mode:
            return [p.copy() for p in frame], 0, 0
        h, w = frame[0].shape
        assert h >= 4 and h % 2 == 0 and w % 2 == 0
        hist = self.hist if self.mode == 2 and self.hist is not None and self.hist[0].shape == frame[0].shape else None
        out, woven = [], 0
        for i, p in enumerate(frame):
            o, wm = deinterlace_plane(p, None if hist is None else hist[i], self.keep)
            out.append(o)
            if i == 0:
                woven = int(wm.sum())
        if self.mode == 2:
            self.hist = [p.copy() for p in frame]
        missing = w * int(((np.arange(h) & 1) != self.keep).sum())
        return out, woven, missing


def _u8(*p):
    return [np.ascontiguousarray(np.clip(x, 0, 255), np.uint8) for x in p]


def sequences(w, h, seed=1, frames=5):
    """name -> list of frames (Y, U, V) uint8 of w x h (chroma w // 2 x h // 2):
    moving: noise plus a drifting picture, nothing stands still; static: one noisy picture again and again; half_static: the left half
    stands still, the right half is new noise every frame"""
    rng = np.random.default_rng(seed)
    cw, ch = w // 2, h // 2

    def pic(t):
        yy, xx = np.mgrid[0:h, 0:w]
        y = 128 + 70 * np.sin((xx - 3 * t) / 4.0) * np.cos((yy + t) / 2.5) + rng.integers(-40, 41, (h, w))
        yy, xx = np.mgrid[0:ch, 0:cw]
        u = 128 + 60 * np.sin((xx + 2 * t) / 3.0 + yy / 2.0) + rng.integers(-30, 31, (ch, cw))
        v = 128 + 60 * np.cos((yy - t) / 2.0) + rng.integers(-30, 31, (ch, cw))
        return _u8(y, u, v)

    seq = {"moving": [pic(t) for t in range(frames)]}
    first = pic(0)
    # (extremes in the static picture: the interpolation's clamp at both ends is exercised where the kept field alternates 0 / 255)
    first[0][:, : max(2, w // 8)] = np.where((np.arange(h)[:, None] // 2) % 2 == 0, 0, 255)
    seq["static"] = [[p.copy() for p in first] for _ in range(frames)]
    half = []
    for t in range(frames):
        f = pic(t + 7)
        for p, q in zip(f, first):
            p[:, : p.shape[1] // 2] = q[:, : p.shape[1] // 2]
        half.append(f)
    seq["half_static"] = half
    return seq


def moving_scene(w, h, t, keep):
    """the interlaced frame of the quality check at time t: the kept field taken at t, the other at t + 1/2; and the progressive frame at t"""
    def luma(tt):
        yy, xx = np.mgrid[0:h, 0:w]
        xs = xx - 2 * tt
        return 128 + 60 * np.sin(xs / 5.0) * np.cos(yy / 3.0) + 25 * (((np.floor(xs).astype(np.int64) >> 3) + (yy >> 2)) & 1)
    prog, other = luma(t), luma(t + 0.5)
    inter = prog.copy()
    inter[1 - keep::2] = other[1 - keep::2]
    c = np.full((h // 2, w // 2), 128)
    return _u8(inter, c, c), _u8(prog, c, c)


def interlaced_video(w, h, n, seed, cut_at=None, keep=0, noise=0, still=16):
    """n interlaced frames for the end-to-end tests: a picture that drifts two samples per frame, the field that is not kept taken
    half a frame later (one sample further); the top `still` luma rows stand still; from cut_at on another picture altogether; noise: the
    amplitude of fresh noise on every frame below the rows that stand still"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w + 2 * n + 2]
    pics = []
    for k in range(2):
        y = 128 + 60 * np.sin((xx + 11 * k) / (5.0 + 4 * k)) * np.cos(yy / (7.0 - 3 * k)) + 25 * (((xx >> 3) + (yy >> 3) + k) & 1) + rng.integers(-3, 4, xx.shape)
        pics.append((y, 128 + 30 * np.sin(xx[:h // 2, :] / 9.0 + k) + yy[:h // 2, :], 128 + 30 * np.cos(yy[:h // 2, :] / 6.0 + 2 * k) + xx[:h // 2, :] % 7))
    out = []
    for t in range(n):
        y, u, v = pics[1 if cut_at is not None and t >= cut_at else 0]
        frame = []
        for p, (pw, ph, step) in zip((y, u, v), ((w, h, 2), (w // 2, h // 2, 1), (w // 2, h // 2, 1))):
            a, b = p[:ph, step * t:step * t + pw].copy(), p[:ph, step * t + step // 2 + step % 2:step * t + step // 2 + step % 2 + pw]
            a[1 - keep::2] = b[1 - keep::2]
            if noise:
                a = a + rng.integers(-noise, noise + 1, a.shape)
            a[:still * ph // h] = p[:still * ph // h, :pw]
            frame.append(a)
        out.append(_u8(*frame))
    return out
