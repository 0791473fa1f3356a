"""The VP8 simple loop filter (RFC 6386 section 15.2), restated on top of the independent decoder in vp8_decode.py.

A frame whose header says filter_type = 1 is filtered here; every other frame goes through the normal filter of the base
class.  Written from the RFC alone: luma only; per macroblock in raster order the left MB edge (mx > 0), the inner vertical
edges 4, 8, 12, the top MB edge (my > 0), the inner horizontal edges; the inner edges are skipped for a macroblock without
non-zero coefficients that is not B_PRED / SPLITMV; a macroblock whose level is 0 is skipped.  Edge test
2|p0-q0| + (|p1-q1| >> 1) <= limit (mbedge limit 2(L+2)+I, sub-block limit 2L+I), then common_adjust(1, ...): only p0 and
q0 change.
"""
import numpy as np

from vp8_decode import Decoder


def simple_edge(P, idx, elim):
    """filter across one edge.  idx: (p1, p0, q0, q1) index arrays selecting the samples along the edge"""
    p1, p0, q0, q1 = [P[i].astype(np.int32) for i in idx]
    mask = (np.abs(p0 - q0) * 2 + (np.abs(p1 - q1) >> 1)) <= elim
    c = lambda v: np.clip(v, -128, 127)
    sp1, sp0, sq0, sq1 = p1 - 128, p0 - 128, q0 - 128, q1 - 128
    a = c(c(sp1 - sq1) + 3 * (sq0 - sp0))
    a = np.where(mask, a, 0)
    f1 = c(a + 4) >> 3
    f2 = c(a + 3) >> 3
    P[idx[2]] = (c(sq0 - f1) + 128).astype(np.uint8)
    P[idx[1]] = (c(sp0 + f2) + 128).astype(np.uint8)


def simple_filter_plane(Y, mbw, mbh, lvl, mbl, sbl, skip_inner):
    """the simple filter over a luma plane, in place.  lvl, mbl, sbl, skip_inner: per macroblock in raster order.
    Macroblocks with the same mx + 2 * my touch disjoint samples and depend only on earlier ones: one vectorised step each."""
    for d in range(mbw + 2 * mbh):
        wave = [(d - 2 * my, my) for my in range(mbh) if 0 <= d - 2 * my < mbw]
        wave = [(mx, my) for mx, my in wave if lvl[my * mbw + mx] > 0]
        if not wave:
            continue

        def run(sel, pos, vertical, lim):
            if not sel:
                return
            ids = np.array([my * mbw + mx for mx, my in sel])
            along = np.concatenate([np.arange(16) + (my if vertical else mx) * 16 for mx, my in sel])
            across = np.repeat(np.array([(mx if vertical else my) * 16 + pos for mx, my in sel]), 16)
            idx = tuple((along, across + k) if vertical else (across + k, along) for k in range(-2, 2))
            simple_edge(Y, idx, np.repeat(lim[ids], 16))

        inner = [(mx, my) for mx, my in wave if not skip_inner[my * mbw + mx]]
        run([(mx, my) for mx, my in wave if mx > 0], 0, True, mbl)
        for x in (4, 8, 12):
            run(inner, x, True, sbl)
        run([(mx, my) for mx, my in wave if my > 0], 0, False, mbl)
        for y in (4, 8, 12):
            run(inner, y, False, sbl)


class SimpleFilterDecoder(Decoder):
    """vp8_decode.Decoder that also decodes frames coded for the simple loop filter"""

    def _loop_filter(self, f, planes, skip_inner):
        if f.filter_type != 1:
            return super()._loop_filter(f, planes, skip_inner)
        n_mb = f.mbw * f.mbh
        lvl = np.zeros(n_mb, np.int32)
        for mb in range(n_mb):
            if f.segmentation_enabled:
                seg = int(f.segment_id[mb])
                l = f.seg_lf[seg] if f.seg_abs else f.loop_filter_level + f.seg_lf[seg]
            else:
                l = f.loop_filter_level
            lvl[mb] = min(max(l, 0), 63)
        il = lvl.copy()
        if f.sharpness:
            il >>= 2 if f.sharpness > 4 else 1
            il = np.minimum(il, 9 - f.sharpness)
        il = np.maximum(il, 1)
        simple_filter_plane(planes[0], f.mbw, f.mbh, lvl, (lvl + 2) * 2 + il, lvl * 2 + il, skip_inner)
