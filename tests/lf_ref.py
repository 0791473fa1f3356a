"""The normal loop filter restated in numpy, in the reference's order and register discipline, with counters of what its inputs reach.

Written from RFC 6386 section 15 (the edge tests of 15.2-15.4, the filters of 15.3/15.4 on pixel - 128) and from what
oracle/vp8_oracle.c's comments say the reference does differently from a decoder (CPU_kernels.cl:970-1075):

  * macroblocks in raster order; per macroblock all vertical edges (the macroblock edge, then the inner ones at 4, 8, 12), then all
    horizontal ones;
  * a line (a pixel row across vertical edges, a column across horizontal ones) is loaded into registers edge by edge: the four
    samples behind an edge are read from the plane, the four in front of an INNER edge are the registers the edge before it left --
    handed on, not read back (:1024, :1062);
  * every edge stores what it changed, and only the store saturates to 0..255.

Two switches:
  carry_saturates    False = the reference: the registers handed to the next edge keep values outside -128..127.  True: they are
                     clamped at the hand-over, which is what a decoder computes (it works on the stored bytes).
  level0_ends_plane  True = the reference (:990): the first macroblock whose segment has loop_filter_level 0 ends the plane.  False =
                     RFC 6386: that macroblock alone is left unfiltered.

Everything is batched over N cases (N tables, and N contents where the planes are (N, H, W)): one numpy operation per step of the
arithmetic for all cases and all lines of a macroblock.  The arithmetic is kept in the RFC's form -- seven separate tests, two clamps
to -128..127 before each `>> 3` -- so that it can disagree with kernels that fold them.

Reach counters (Reach.n[kind][name], kind 'mb' = macroblock edge, 'inner' = inner edge; one count per case, in lines of edges that
are applied), named by what sits exactly where:
  edge_at_E / edge_at_E1      2|p0-q0| + (|p1-q1| >> 1) == E / E + 1 while every interior test passes: the edge test decides
  int_at_I / int_at_I1        the largest of the six interior differences == I / I + 1 while the edge test passes
  hev_at_T / hev_at_T1        max(|p1-p0|, |q1-q0|) == hev_thr / hev_thr + 1 while the mask passes
  c1_lo / c1_hi               p1 - q1 below -128 / above 127 where the first clamp's result is used and the mask passes
  c2_lo / c2_hi               the sum the second clamp takes below -128 / above 127 while the mask passes
  shortcut                    the filter value in 124..127: a + 4 and a + 3 both pass 127 before their `>> 3`
  carry_lo / carry_hi         a register handed on by an edge of this kind below -128 / above 127
"""
import numpy as np

SD_LEVEL, SD_MBEDGE_LIMIT, SD_SUB_BEDGE_LIMIT, SD_INTERIOR_LIMIT, SD_HEV_THRESHOLD = 6, 7, 8, 9, 10
KINDS = ("mb", "inner")
NAMES = ("edge_at_E", "edge_at_E1", "int_at_I", "int_at_I1", "hev_at_T", "hev_at_T1", "c1_lo", "c1_hi", "c2_lo", "c2_hi", "shortcut",
         "carry_lo", "carry_hi")


class Reach:
    def __init__(self, n_cases):
        self.n = {k: {name: np.zeros(n_cases, np.int64) for name in NAMES} for k in KINDS}

    def add(self, kind, name, where):
        self.n[kind][name] += where.sum(axis=1)

    def total(self, kind, name):
        return int(self.n[kind][name].sum())


def _c(v):
    return np.clip(v, -128, 127)


def _edge(p3, p2, p1, p0, q0, q1, q2, q3, E, I, T, mb_edge, gate, reach):
    """One edge on signed samples.  Returns the changed registers, unsaturated: (p2, p1, p0, q0, q1, q2) of a macroblock edge,
    (p1, p0, q0, q1) of an inner edge."""
    a = np.abs
    interior = np.maximum.reduce([a(p3 - p2), a(p2 - p1), a(p1 - p0), a(q1 - q0), a(q2 - q1), a(q3 - q2)])
    edge = a(p0 - q0) * 2 + (a(p1 - q1) >> 1)
    mask = (interior <= I) & (edge <= E)
    var = np.maximum(a(p1 - p0), a(q1 - q0))
    hev = var > T
    d1 = p1 - q1
    if mb_edge:
        s = _c(d1) + 3 * (q0 - p0)
        w = np.where(mask, _c(s), 0)
        f = np.where(hev, w, 0)              # high edge variance: the inner two samples only
        used1 = True
        nq0, np0 = q0 - (_c(f + 4) >> 3), p0 + (_c(f + 3) >> 3)
        w = np.where(hev, 0, w)
        t = _c((27 * w + 63) >> 7)
        nq0, np0 = nq0 - t, np0 + t
        t = _c((18 * w + 63) >> 7)
        nq1, np1 = q1 - t, p1 + t
        t = _c((9 * w + 63) >> 7)
        out = (p2 + t, np1, np0, nq0, nq1, q2 - t)
    else:
        s = np.where(hev, _c(d1), 0) + 3 * (q0 - p0)
        f = np.where(mask, _c(s), 0)
        used1 = hev
        f1 = _c(f + 4) >> 3
        nq0, np0 = q0 - f1, p0 + (_c(f + 3) >> 3)
        t = np.where(hev, 0, (f1 + 1) >> 1)
        out = (p1 + t, np0, nq0, q1 - t)
    if reach is not None:
        k = "mb" if mb_edge else "inner"
        inner_ok, edge_ok = gate & (interior <= I), gate & (edge <= E)
        m = gate & mask
        reach.add(k, "edge_at_E", inner_ok & (edge == E))
        reach.add(k, "edge_at_E1", inner_ok & (edge == E + 1))
        reach.add(k, "int_at_I", edge_ok & (interior == I))
        reach.add(k, "int_at_I1", edge_ok & (interior == I + 1))
        reach.add(k, "hev_at_T", m & (var == T))
        reach.add(k, "hev_at_T1", m & (var == T + 1))
        reach.add(k, "c1_lo", m & used1 & (d1 < -128))
        reach.add(k, "c1_hi", m & used1 & (d1 > 127))
        reach.add(k, "c2_lo", m & (s < -128))
        reach.add(k, "c2_hi", m & (s > 127))
        reach.add(k, "shortcut", gate & (f >= 124))
    return out


def _lines(t, n, has_mb_edge, lim, gate_mb, gate_in, carry_saturates, reach):
    """t: (N, lines, 4 + n) signed samples of the plane (a view: the stores go through), t[..., 0:4] in front of the macroblock edge
    (absent -- t is (N, lines, n) -- where the macroblock has no such edge)."""
    E_mb, E_b, I, T = lim
    o = 4 if has_mb_edge else 0

    def store(k, v, gate):
        t[:, :, o + k] = np.where(gate, _c(v), t[:, :, o + k])     # signed -128..127 is the byte 0..255

    q0, q1, q2, q3 = (t[:, :, o + k].copy() for k in range(4))
    if has_mb_edge:
        p3, p2, p1, p0 = (t[:, :, k].copy() for k in range(4))
        p2, p1, p0, q0, q1, q2 = _edge(p3, p2, p1, p0, q0, q1, q2, q3, E_mb, I, T, True, gate_mb, reach)
        for k, v in zip((-3, -2, -1, 0, 1, 2), (p2, p1, p0, q0, q1, q2)):
            store(k, v, gate_mb)
    for e in range(4, n, 4):
        if reach is not None:
            k = "mb" if e == 4 else "inner"
            if e > 4 or has_mb_edge:
                reach.add(k, "carry_lo", gate_in & ((q0 < -128) | (q1 < -128) | (q2 < -128)))
                reach.add(k, "carry_hi", gate_in & ((q0 > 127) | (q1 > 127) | (q2 > 127)))
        p3, p2, p1, p0 = q0, q1, q2, q3            # handed on, not read back
        if carry_saturates:
            p3, p2, p1, p0 = _c(p3), _c(p2), _c(p1), _c(p0)
        q0, q1, q2, q3 = (t[:, :, o + e + k].copy() for k in range(4))
        p1, p0, q0, q1 = _edge(p3, p2, p1, p0, q0, q1, q2, q3, E_b, I, T, False, gate_in, reach)
        for k, v in zip((-2, -1, 0, 1), (p1, p0, q0, q1)):
            store(e + k, v, gate_in)


class Filtered:
    """planes: (Y, U, V) uint8, (N, H, W) each; filtered: (N, macroblocks) bool, the macroblocks that were filtered; reach: Reach or None"""

    def __init__(self, planes, filtered, reach):
        self.planes, self.filtered, self.reach = planes, filtered, reach


def loop_filter(planes, seg, inner, sd, carry_saturates=False, level0_ends_plane=True, count=False):
    """planes: (Y, U, V), each (H, W) or (N, H, W) uint8; seg: (macroblocks,) or (N, macroblocks) segment ids; inner: the same shape,
    non-zero where the macroblock's inner edges are filtered (the filter mask); sd: (4, 11) or (N, 4, 11) segment data."""
    sd = np.asarray(sd, np.int64)
    sd = sd.reshape((-1, 4, 11))
    N = max(sd.shape[0], *(p.shape[0] if p.ndim == 3 else 1 for p in planes), np.atleast_2d(seg).shape[0])
    sd = np.broadcast_to(sd, (N, 4, 11))
    seg = np.broadcast_to(np.atleast_2d(np.asarray(seg, np.int64)), (N, np.asarray(seg).shape[-1]))
    inner = np.broadcast_to(np.atleast_2d(np.asarray(inner) != 0), seg.shape)
    H, W = planes[0].shape[-2:]
    mbw, mbh = W // 16, H // 16
    ar = np.arange(N)
    reach = Reach(N) if count else None
    out = []
    filtered = np.zeros((N, mbw * mbh), bool)
    for P, n in zip(planes, (16, 8, 8)):
        A = np.array(np.broadcast_to(P, (N,) + P.shape[-2:]), np.int32) - 128
        ended = np.zeros(N, bool)
        for mb in range(mbw * mbh):
            s = seg[:, mb]
            zero = sd[ar, s, SD_LEVEL] == 0
            if level0_ends_plane:
                ended |= zero
                active = ~ended
                if ended.all():
                    break
            else:
                active = ~zero
            if not active.any():
                continue
            filtered[:, mb] = active
            lim = tuple(sd[ar, s, k].astype(np.int32)[:, None] for k in (SD_MBEDGE_LIMIT, SD_SUB_BEDGE_LIMIT, SD_INTERIOR_LIMIT, SD_HEV_THRESHOLD))
            gate_mb, gate_in = active[:, None], (active & inner[:, mb])[:, None]
            x0, y0 = (mb % mbw) * n, (mb // mbw) * n
            _lines(A[:, y0:y0 + n, x0 - 4 if x0 else 0:x0 + n], n, x0 > 0, lim, gate_mb, gate_in, carry_saturates, reach)
            _lines(A[:, y0 - 4 if y0 else 0:y0 + n, x0:x0 + n].transpose(0, 2, 1), n, y0 > 0, lim, gate_mb, gate_in, carry_saturates, reach)
        out.append((A + 128).astype(np.uint8))
    return Filtered(tuple(out), filtered, reach)
