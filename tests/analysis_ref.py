"""The two rules of the frame analysis record (vp8hip_set_analysis) restated in numpy from the text of include/vp8hip_host.h alone.
Everything is an exact integer: Python ints, no floats."""
import numpy as np

SOURCE_FIELDS = ("have_prev", "static_mbs", "spatial", "temporal_sse", "temporal_sad")
CODING_FIELDS = ("mbs_total", "mbs_intra", "mbs_split", "mbs_zero_mv", "mbs_no_coeffs", "mbs_ref", "segment_mbs", "mv_abs_sum", "mv_sum",
                 "mv_sq_sum", "nz_coeffs")


def _blocks(plane):
    """[MB rows][MB columns][256] int64 of a plane whose sides are whole macroblocks"""
    h, w = plane.shape
    assert h >= 16 and w >= 16 and h % 16 == 0 and w % 16 == 0
    return plane.astype(np.int64).reshape(h // 16, 16, w // 16, 16).transpose(0, 2, 1, 3).reshape(h // 16, w // 16, 256)


def source_side(cur, prev=None) -> dict:
    """cur, prev: the luma plane at the coded size (uint8) of this frame and of the previous frame taken in (None: no history)"""
    x = _blocks(np.asarray(cur))
    s, ss = x.sum(axis=2), (x * x).sum(axis=2)
    out = {"spatial": int((256 * ss - s * s).sum()), "temporal_sse": 0, "temporal_sad": 0, "static_mbs": 0, "have_prev": 0}
    if prev is not None:
        d = x - _blocks(np.asarray(prev))
        out.update(have_prev=1, temporal_sse=int((d * d).sum()), temporal_sad=int(np.abs(d).sum()),
                   static_mbs=int((np.abs(d).sum(axis=2) == 0).sum()))
    return out


def coding_side(is_key, parts, ref, vec, nz, seg, is_inter=None) -> dict:
    """the per-macroblock arrays of the frame's final coding attempt, raster order.  is_inter: the flags of check_SSIM's fallback when
    they count (an inter frame, the check ran and reported replaced > 0), else None"""
    nz, seg = np.asarray(nz, np.int64), np.asarray(seg, np.int64) & 3
    n = nz.size
    if is_key:
        inter = np.zeros(n, bool)
    elif is_inter is None:
        inter = np.ones(n, bool)
    else:
        inter = np.asarray(is_inter) != 0
    v = np.asarray(vec, np.int64).reshape(n, 4, 2)[inter]
    ref, parts = np.asarray(ref)[inter], np.asarray(parts)[inter]
    return {
        "mbs_total": n,
        "mbs_intra": int((~inter).sum()),
        "mbs_ref": [int((ref == r).sum()) for r in range(3)],
        "mbs_split": int((parts == 1).sum()),
        "mbs_zero_mv": int((np.abs(v).reshape(-1, 8).sum(axis=1) == 0).sum()),
        "mv_abs_sum": [int(np.abs(v[:, :, k]).sum()) for k in range(2)],
        "mv_sum": [int(v[:, :, k].sum()) for k in range(2)],
        "mv_sq_sum": int((v * v).sum()),
        "nz_coeffs": int(nz.sum()),
        "mbs_no_coeffs": int((nz == 0).sum()),
        "segment_mbs": [int((seg == s).sum()) for s in range(4)],
    }


def planes(w, h, kind, seed=0):
    """test luma planes"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "constant":
        return np.full((h, w), 77, np.uint8)
    if kind == "extremes":      # every sample 0 or 255: the widest sums there are
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    raise ValueError(kind)


def video(w, h, n, seed=0, still_from=None):
    """n I420 frames: a textured picture that drifts a sample per frame under light noise, with a still strip on the left third of
    pictures at least three macroblocks wide (static macroblocks); from `still_from` on the frame repeats exactly"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w + n + 8]
    base = 128 + 70 * np.sin(xx / 4.3) * np.cos(yy / 5.1) + 30 * (((xx >> 2) + (yy >> 3)) & 1)
    cu, cv = 128 + 40 * np.sin(xx[:h // 2, :] / 7.0), 128 + 40 * np.cos(yy[:h // 2, :] / 5.0)
    out = []
    for t in range(n):
        if still_from is not None and t > still_from:
            out.append(tuple(p.copy() for p in out[-1]))
            continue
        y = base[:, t:t + w] + rng.integers(-3, 4, (h, w))
        still = (w // 48) * 16      # (no strip in pictures narrower than three macroblocks)
        y[:, :still] = base[:, :still]
        u, v = cu[:, t // 2:t // 2 + w // 2], cv[:, t // 2:t // 2 + w // 2]
        out.append(tuple(np.ascontiguousarray(np.clip(p, 0, 255), dtype=np.uint8) for p in (y, u, v)))
    return out


def noisy_still(w, h, n, seed=0):
    """n I420 frames of ONE picture under fresh noise of amplitude 3 per frame: what a temporal denoiser does filter"""
    rng = np.random.default_rng(seed)
    base = video(w, h, 1, seed=seed)[0]
    return [tuple(np.clip(p.astype(int) + rng.integers(-3, 4, p.shape), 0, 255).astype(np.uint8) for p in base) for _ in range(n)]
