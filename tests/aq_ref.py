"""The variance-adaptive segment map (vp8hip_set_segment_mode, mode 2) restated in numpy from the rule in include/vp8hip_host.h:
all integers.  aq_map(luma, strength, width=None) -> (map, e, E), one entry per macroblock in raster order."""
import numpy as np

AQ_W = {1: 24, 2: 16, 3: 12}


def mb_e(luma: np.ndarray, width=None) -> np.ndarray:
    """e(mb) = log2(v + 1) in eighths, piecewise linear, v = 256 * sum x^2 - (sum x)^2 over the macroblock's 256 samples"""
    luma = np.asarray(luma)
    h = luma.shape[0]
    w = luma.shape[1] if width is None else width
    assert w % 16 == 0 and h % 16 == 0 and w >= 16 and h >= 16
    x = luma[:, :w].astype(np.int64).reshape(h // 16, 16, w // 16, 16)
    s = x.sum(axis=(1, 3))
    ss = (x * x).sum(axis=(1, 3))
    v = (256 * ss - s * s).reshape(-1)
    e = np.zeros(v.size, np.int64)
    for i, vi in enumerate(v):
        n = int(vi) + 1
        p = n.bit_length() - 1
        frac = (n >> (p - 3)) & 7 if p >= 3 else (n << (3 - p)) & 7
        e[i] = 8 * p + frac
    return e


def segments_of(e: np.ndarray, strength: int):
    E = int(e.sum()) // e.size
    seg = np.clip(2 + np.floor_divide(e - E, AQ_W[strength]), 0, 3)      # numpy's floor_divide rounds towards minus infinity
    return seg.astype(np.uint8), E


def aq_map(luma: np.ndarray, strength: int, width=None):
    e = mb_e(luma, width)
    seg, E = segments_of(e, strength)
    return seg, e.astype(np.uint8), E


def noise_blocks(w: int, h: int, amplitudes=(3, 6, 12, 24), seed: int = 0) -> np.ndarray:
    """macroblocks of uniform noise around 128, the amplitude cycling through `amplitudes` in raster order"""
    rng = np.random.default_rng(seed)
    y = np.zeros((h, w), np.uint8)
    k = 0
    for my in range(h // 16):
        for mx in range(w // 16):
            a = amplitudes[k % len(amplitudes)]
            y[my * 16:my * 16 + 16, mx * 16:mx * 16 + 16] = 128 + rng.integers(-a, a + 1, (16, 16))
            k += 1
    return y
