"""The batched quarter-pel search with its filter bytes packed without permutes (round_pack4: the second v_ashr_pk_i8_i32 of a pair writes
the upper half of the first one's register) and its result written by the winning lane (kernels_s2.hip), through two test taps.

1. vp8hip_debug_round_pack4 against numpy: sat_i8(x >> 7) per element, element j of a quadruple in byte j.  Values: INT32_MIN, INT32_MAX, 0,
   +-1, every value of +-(128 * 128 +- 130) (around the two saturation points +-16384 and past them), and 4096 random int32 (+ 4096 random values
   inside the filter's range); every special value meets every byte position under both polarities of the neighbouring half (the other half of
   the dword saturating the other way: what a half that is not preserved would show), and all 81 quadruples of {below, inside, above} meet.
2. vp8hip_debug_search2_batch against vp8o_luma_search_2step on the same planes and whole-pel nets, vectors and costs bit for bit:
   shapes 16x16 (4 blocks: half a group), 48x32 (24 blocks: one and a half workgroups of two groups), 176x144; four members with 1, 2, 3 and
   2 (LAST + ALTREF: a gap in the map) references in one launch, and the three-reference member as a batch of one; whole-pel nets of three kinds
   (random vectors that keep the window in the frame; all zero; vectors that put every candidate of some blocks out of the frame, the int16
   extremes among them); content: a panned random texture, a noise frame against its inverse, 0 / 255 stripes of period 2 and 3 along x and y
   (two setups per shape, so that every content meets two reference counts).  The references are plain uploads (GOLDEN and ALTREF rotated in
   from LAST), so the oracle's planes are the uploaded ones; the device's planes are read back and compared first.
3. What the cases reach, from the oracle alone (no GPU: test_the_cases_reach_what_they_are_here_for):
   - blocks won by the zero candidate while a non-zero whole-pel vector stood, and blocks whose 25 offset candidates ALL lie out of the frame
     (only the zero candidate is left);
   - the striped content takes the six-tap sums of both passes below 0 and above 255 before the clamp (a numpy restatement of the passes).
   Two more cases were asked for, cannot occur, and are asserted ABSENT, each with the reason asserted beside it:
   - a block that ends on the frame's last position (:1136-1137, cost 0x7fff: no candidate accepted).  The zero candidate is in the frame for every
     block of the frame, so this needs a zero-vector cost of 0x7fff or more; the metric of a 4x4 block is a sum of absolute values of (rounded) linear
     forms of the differences, so it is largest at a corner of [-255, 255]^16, and over all 65536 corners it reaches 7266: four blocks stay under
     29100 (test_no_block_can_cost_0x7fff walks the corners through the oracle's own vp8o_weight).  The kernel keeps the case behind a branch.
   - a vector of (0, 0) reached through a NON-ZERO offset: the whole-pel vector enters in quarter pels, (int16)(4 n), a multiple of 4 also after
     the wrap, and the offsets are -2..2, so v0 + d = 0 only for v0 = 0 and d = 0.  What stands in for it is its neighbour: blocks whose whole-pel
     vector is zero and whose winner is the zero OFFSET (candidate 12, which ties with the zero candidate and precedes it) -- the (0, 0) result
     whose cost is what the key holds.
Run with `pytest -m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle_lib import Oracle
from pipeline import default_segments
from vp8oclenc_amd import api

SHAPES = [(16, 16), (48, 32), (176, 144)]
FLAGS = [(0, 0), (1, 0), (1, 1), (0, 1)]      # (use_golden, use_altref) per member, as in test_gpu_search2_ref_loop.py
ONE = 2                                        # the member that also runs as a batch of one: three references
NETS = ("in the frame", "zero", "out of the frame")
CONTENTS = ("texture", "inverse", "stripes a", "stripes b")
SETUPS = (0, 2)                                # member i of setup s has content (i + s) % 4
EXTREMES = (32767, -32768, -32767, 32766, -32766, 16384, -16384, 8191, -8192, 8190, -8191, 4097, -4097, 2049)
TAPS = {1: (1, -8, 36, 108, -11, 2), 2: (3, -16, 77, 77, -16, 3), 3: (2, -11, 108, 36, -8, 1)}     # quarter-pel phases 1..3, GPU_kernels.cl:563-572


# ---- round_pack4 -------------------------------------------------------------------------------------------------------------------
def _pack_values():
    special = [-2 ** 31, 2 ** 31 - 1, 0, 1, -1]
    for s in (1, -1):
        special += [s * (128 * 128 + d) for d in range(-130, 131)]
    lo, hi = -(1 << 20), 1 << 20                 # saturate below / above
    quads = []
    for v in special:
        for pos in range(4):
            for fill in ((hi, hi, lo, lo), (lo, lo, hi, hi)):      # the two halves of the dword saturate in opposite directions
                q = list(fill)
                q[pos] = v
                quads.append(q)
    kinds = (lo, 1234, hi)
    quads += [[kinds[(i // 3 ** j) % 3] for j in range(4)] for i in range(81)]      # every direction meets every byte position
    rng = np.random.default_rng(20260)
    quads += rng.integers(-2 ** 31, 2 ** 31, size=(1024, 4)).tolist()
    quads += rng.integers(-20000, 20001, size=(1024, 4)).tolist()
    return np.ascontiguousarray(np.array(quads, np.int64).astype(np.int32))


@pytest.mark.gpu
def test_round_pack4_is_sat_i8_of_x_shifted_by_7_in_every_byte():
    v = _pack_values()
    n = len(v)
    out = np.full(n, 0x5a5a5a5a, np.uint32)
    hip = api.Vp8Hip(16, 16)
    try:
        rc = hip.lib.vp8hip_debug_round_pack4(hip.h, C.c_void_p(v.ctypes.data), n, C.c_void_p(out.ctypes.data))
    finally:
        hip.close()
    assert rc == 0, rc
    b = np.clip(v.astype(np.int64) >> 7, -128, 127) & 255
    want = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)).astype(np.uint32)
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, (bad.size, [(v[i].tolist(), hex(int(out[i])), hex(int(want[i]))) for i in bad[:5]])


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _stripes(W, H, period, along_x, bright=1):
    """0 / 255 stripes: `bright` of every `period` lines are 255 (one bright line in three undershoots the six taps, two in three overshoot them)"""
    i = np.arange(W if along_x else H)
    line = np.where(i % period < bright, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(line[None, :] if along_x else line[:, None], (H, W)))


@functools.lru_cache(maxsize=None)
def _content(W, H, kind):
    """(current, [LAST, GOLDEN, ALTREF]) luma planes"""
    rng = np.random.default_rng(1000 * W + H + 7 * CONTENTS.index(kind))
    if kind == "texture":
        m = 16
        hh, ww = H + 2 * m, W + 2 * m
        coarse = rng.integers(40, 216, size=(hh // 4 + 1, ww // 4 + 1))
        canvas = np.clip(np.kron(coarse, np.ones((4, 4), np.int64))[:hh, :ww] + rng.integers(-20, 21, size=(hh, ww)), 0, 255).astype(np.uint8)
        cut = lambda dx, dy: np.ascontiguousarray(canvas[m + dy:m + dy + H, m + dx:m + dx + W])
        return cut(0, 0), [cut(1, 0), cut(-2, 1), cut(0, -1)]
    if kind == "inverse":
        f = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
        g = np.clip(f.astype(np.int64) + rng.integers(-3, 4, size=(H, W)), 0, 255).astype(np.uint8)
        return f, [np.ascontiguousarray(255 - f), g, np.ascontiguousarray(255 - g)]
    if kind == "stripes a":
        return _stripes(W, H, 2, True), [_stripes(W, H, 3, True), _stripes(W, H, 2, False), _stripes(W, H, 3, False, 2)]
    return _stripes(W, H, 2, False), [_stripes(W, H, 2, True), _stripes(W, H, 3, False), _stripes(W, H, 3, True, 2)]


def _net(W, H, kind, seed):
    """a whole-pel net: (b8, 2) int16, cell b = the vector of 8x8 block b (row by row)"""
    rng = np.random.default_rng(seed)
    bw, bh = W // 8, H // 8
    net = np.zeros((bw * bh, 2), np.int16)
    if kind == "zero":
        return net
    for b in range(bw * bh):
        cx, cy = 8 * (b % bw), 8 * (b // bw)
        net[b] = (rng.integers(max(-cx, -12), min(W - 8 - cx, 12) + 1), rng.integers(max(-cy, -12), min(H - 8 - cy, 12) + 1))
        if kind == "out of the frame" and b % 3 != 2:      # along one axis, or along both
            for k in range(2):
                if b % 5 == 0 or k == b % 2:
                    net[b, k] = EXTREMES[(b + k + seed) % len(EXTREMES)]
    return net


def _use(flags):
    return [1, flags[0], flags[1]]


@functools.lru_cache(maxsize=None)
def oracle_cases(W, H, setup):
    """{(member, net kind, reference): (whole-pel net, the oracle's quarter-pel net, the oracle's costs)}, from the CPU oracle alone"""
    st = Oracle.stages()
    res = {}
    for i, flags in enumerate(FLAGS):
        cur, refs = _content(W, H, CONTENTS[(i + setup) % 4])
        for kn, kind in enumerate(NETS):
            for r in range(3):
                if not _use(flags)[r]:
                    continue
                net = _net(W, H, kind, 100 * setup + 10 * i + r + W)
                want = np.zeros_like(net)
                cost = np.zeros(len(net), np.int32)
                st.luma_search_2step(cur, refs[r], net, want, cost, W, H)
                res[(i, kind, r)] = (net, want, cost)
    return res


def _six_tap_range(plane):
    """(min, max) of the rounded six-tap results BEFORE the clamp over the three fractional phases: the horizontal pass over the plane, and the
    vertical pass over the horizontal pass's clamped results and over the plane itself (the whole-pel x case)"""
    def one_pass(a, axis):
        a = a.astype(np.int64)
        lo, hi, outs = 1 << 30, -(1 << 30), []
        n = a.shape[axis]
        for taps in TAPS.values():
            s = sum(t * np.take(a, np.arange(j, n - 5 + j), axis=axis) for j, t in enumerate(taps))
            s = (s + 64) >> 7
            lo, hi = min(lo, int(s.min())), max(hi, int(s.max()))
            outs.append(np.clip(s, 0, 255))
        return lo, hi, outs
    hlo, hhi, hs = one_pass(plane, 1)
    vlo, vhi = 1 << 30, -(1 << 30)
    for a in hs + [plane]:
        lo, hi, _ = one_pass(a, 0)
        vlo, vhi = min(vlo, lo), max(vhi, hi)
    return (hlo, hhi), (vlo, vhi)


@functools.lru_cache(maxsize=None)
def reach(W, H):
    """what the cases of one shape reach, from the oracle's results: a dict of counts"""
    bw = W // 8
    n = dict(last_position=0, zero_candidate=0, zero_by_nonzero_offset=0, zero_offset_on_zero_vector=0, only_zero_candidate_in_frame=0)
    for setup in SETUPS:
        for (i, kind, r), (net, want, cost) in oracle_cases(W, H, setup).items():
            for b in range(len(net)):
                cx4, cy4 = 32 * (b % bw), 32 * (b // bw)
                v0x, v0y = (int(v) for v in (net[b].astype(np.int32) * 4).astype(np.int16))
                lx, ly = (int(v) for v in np.array([4 * W - 32 - cx4, 4 * H - 32 - cy4]).astype(np.int16))
                vx, vy, c = int(want[b, 0]), int(want[b, 1]), int(cost[b])
                pen = (abs(vx - v0x) + abs(vy - v0y)) * 32 if (vx or vy) else 0
                qx = [int(np.array(cx4 + v0x + d).astype(np.int16)) for d in range(-2, 3)]
                qy = [int(np.array(cy4 + v0y + d).astype(np.int16)) for d in range(-2, 3)]
                if not any(0 <= x <= 4 * W - 32 for x in qx) or not any(0 <= y <= 4 * H - 32 for y in qy):
                    n["only_zero_candidate_in_frame"] += 1
                if c == 0x7fff - pen and (vx, vy) == (lx, ly):
                    n["last_position"] += 1
                elif (vx, vy) == (0, 0):
                    if (v0x, v0y) != (0, 0):
                        n["zero_candidate"] += 1
                        n["zero_by_nonzero_offset"] += int(abs(v0x) <= 2 and abs(v0y) <= 2)
                    else:
                        n["zero_offset_on_zero_vector"] += 1      # candidate 12 (it precedes the zero candidate, which ties with it)
    return n


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_cases_reach_what_they_are_here_for(W, H):
    """on the CPU, from the oracle and a numpy restatement of the two passes"""
    n = reach(W, H)
    print(f"{W}x{H}: {n}")
    assert n["zero_candidate"] > 0 and n["only_zero_candidate_in_frame"] > 0, n
    assert n["last_position"] == 0, n                     # cannot occur (see the head of the file and test_no_block_can_cost_0x7fff)
    assert n["zero_by_nonzero_offset"] == 0, n            # cannot occur either ...
    assert n["zero_offset_on_zero_vector"] > 0, n         # ... its neighbour does
    hr, vr = (1 << 30, -(1 << 30)), (1 << 30, -(1 << 30))
    for kind in ("stripes a", "stripes b"):
        for plane in _content(W, H, kind)[1]:
            (hl, hh), (vl, vh) = _six_tap_range(plane)
            hr, vr = (min(hr[0], hl), max(hr[1], hh)), (min(vr[0], vl), max(vr[1], vh))
    print(f"{W}x{H}: six-tap results before the clamp: horizontal pass {hr}, vertical pass {vr}")
    assert hr[0] < 0 and hr[1] > 255 and vr[0] < 0 and vr[1] > 255, (hr, vr)


def test_no_block_can_cost_0x7fff():
    """every corner of [-255, 255]^16 through the oracle's metric: four 4x4 blocks stay far below 0x7fff, so the zero candidate -- in the frame for
    every block -- is always accepted and no block ends on the frame's last position"""
    lib = Oracle.lib()
    d = np.zeros(16, np.int32)
    top = 0
    for pat in range(1 << 16):
        d[:] = [255 if (pat >> j) & 1 else -255 for j in range(16)]
        top = max(top, lib.vp8o_weight(d))
    print(f"largest 4x4 metric over the 65536 corners: {top}")
    assert 4 * (top + 64) < 0x7fff, top      # (+ 64: more than the roundings of the 32 linear forms can add inside the cube)


# ---- the device ----------------------------------------------------------------------------------------------------------------------
def _prepare(be, cur, refs):
    """refs[1] GOLDEN, refs[2] ALTREF, refs[0] LAST through the reference's own rotation rules (each a plain upload); then the current frame, and one
    search over them, which leaves LAST's replicated edges standing"""
    grey = np.full((cur.shape[0] // 2, cur.shape[1] // 2), 128, np.uint8)
    be.upload_last(refs[1], grey, grey)
    be.upload_current(cur, grey, grey)
    be.inter_transform(1, 0, 0, 0)
    be.loop_filter()
    be.upload_last(refs[2], grey, grey)
    be.upload_current(cur, grey, grey)
    be.inter_transform(0, 1, 0, 0)
    be.loop_filter()
    be.upload_last(refs[0], grey, grey)
    be.upload_current(cur, grey, grey)
    be.inter_transform(0, 0, 1, 1)


def _differences(W, H):
    """[(setup, way, member, net kind, reference, what, how many)] where the tap's results are not the oracle's"""
    lib = api.load_library()
    lib.vp8hip_debug_search2_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_void_p)] * 3
    sd = default_segments()
    bad = []
    for setup in SETUPS:
        want = oracle_cases(W, H, setup)
        members = [api.Vp8Hip(W, H) for _ in FLAGS]
        try:
            for i, m in enumerate(members):
                cur, refs = _content(W, H, CONTENTS[(i + setup) % 4])
                m.set_segments(sd)
                _prepare(m, cur, refs)
                for r, plane in ((3, cur), (0, refs[0]), (1, refs[1]), (2, refs[2])):
                    if not np.array_equal(np.asarray(m.debug(api.DBG_PYRAMID, r, 0)), plane):
                        bad.append((setup, "planes", i, "", r, "the device's plane is not the uploaded one", 0))
            api.device_synchronize()
            for way, idx in (("batch of 4", list(range(len(FLAGS)))), ("batch of 1", [ONE])):
                n = len(idx)
                for kind in NETS:
                    src, dst, cost = {}, {}, {}
                    for k, i in enumerate(idx):
                        for r in range(3):
                            if _use(FLAGS[i])[r]:
                                src[(k, r)] = np.ascontiguousarray(want[(i, kind, r)][0])
                                dst[(k, r)] = np.full_like(src[(k, r)], 0x3333)
                                cost[(k, r)] = np.full(len(src[(k, r)]), 0x33333333, np.int32)
                    ptr = lambda d: (C.c_void_p * (3 * n))(*[d[(k, r)].ctypes.data if (k, r) in d else None for k in range(n) for r in range(3)])
                    ints = lambda v: (C.c_int * n)(*v)
                    rc = lib.vp8hip_debug_search2_batch((C.c_void_p * n)(*[members[i].h for i in idx]), n, ints([FLAGS[i][0] for i in idx]),
                                                        ints([FLAGS[i][1] for i in idx]), ptr(src), ptr(dst), ptr(cost))
                    assert rc == 0, rc
                    for (k, r) in src:
                        _, wnet, wcost = want[(idx[k], kind, r)]
                        for what, got, exp in (("vectors", dst[(k, r)], wnet), ("costs", cost[(k, r)], wcost)):
                            if not np.array_equal(got, exp):
                                bad.append((setup, way, idx[k], kind, r, what, int((got != exp).sum())))
        finally:
            for m in members:
                m.close()
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SHAPES)
def test_the_search_over_written_nets_gives_the_oracles_vectors_and_costs(W, H):
    test_the_cases_reach_what_they_are_here_for(W, H)      # (what is compared reaches what it is here for: asserted first)
    bad = _differences(W, H)
    assert not bad, bad[:20]
