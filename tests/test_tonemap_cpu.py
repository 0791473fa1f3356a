"""The tone-mapping rule on the host (vp8host_tonemap_tables, vp8host_tonemap_frame; include/vp8hip_host.h): the tables against
numpy's own evaluation of their formulas, the properties the header promises, and the plain C++ form against the numpy restatement
(tests/tonemap_ref.py) and against the BGRA rule on the restatement's c8 picture, byte for byte.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import tonemap_ref as T
from vp8oclenc_amd import api

PAIRS = [(T.PQ, 1000), (T.PQ, 4000), (T.PQ, 10000), (T.HLG, 1000), (T.HLG, 400)]
SIZES = [(2, 2), (18, 10), (34, 6), (130, 66)]


@pytest.fixture(scope="module")
def host_tables():
    return {pair: api.tonemap_tables(*pair) for pair in PAIRS}


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
# +-1: two evaluations of the same double expression, each correct to an ulp or so, can land on either side of a rounding boundary, by
# one and no more
@pytest.mark.parametrize("pair", PAIRS)
def test_tables_agree_with_numpys_evaluation(host_tables, pair):
    lin, gain, lo, hi = (t.astype(np.int64) for t in host_tables[pair])
    rlin, rgain, rlo, rhi = T.tables_ref(*pair)
    for name, a, b in (("lin", lin, rlin), ("lo", lo, rlo), ("hi", hi, rhi), ("grey o", T.grey_o(lin, gain), T.grey_o(rlin, rgain))):
        worst = int(np.abs(a - b).max())
        print(f"{pair} {name}: largest difference {worst}")
        assert worst <= 1, (pair, name, worst)


@pytest.mark.parametrize("pair", PAIRS)
def test_table_properties(host_tables, pair):
    lin, gain, lo, hi = (t.astype(np.int64) for t in host_tables[pair])
    o = T.grey_o(lin, gain)
    c8 = T.c8_of(o, lo, hi)
    assert np.all(np.diff(lin) >= 0) and np.all(np.diff(o) >= 0) and np.all(np.diff(c8) >= 0)
    assert lin[0] == 0 and c8[4095] == 255
    assert gain.max() < 2 ** 23 and lin.max() < 2 ** 20
    assert np.all(T.PRIMARIES.sum(axis=1) == 1024)


# ---- the frame ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("matrix", range(4))
@pytest.mark.parametrize("fmt", [T.P010, T.I010])
def test_frame_equals_the_restatement_and_the_bgra_rule(host_tables, fmt, matrix, size):
    w, h = size
    pair = PAIRS[(matrix + (fmt == T.I010)) % len(PAIRS)]      # (every pair meets both formats; all pairs at every size: the GPU test's host side)
    for name, y, cb, cr in T.inputs(w, h):
        planes = T.make_planes(fmt, y, cb, cr)
        got = api.tonemap_frame(fmt, pair[0], pair[1], w, h, planes, matrix)
        c8 = T.c8_picture(y, cb, cr, host_tables[pair])
        want = T.i420_of(c8, matrix)
        via_bgra = api.convert_frame(T.BGRA, w, h, [T.bgra_of(c8)], matrix)
        for p, g, r, b in zip("YUV", got, want, via_bgra):
            assert np.array_equal(g, r), (name, pair, p, "restatement")
            assert np.array_equal(g, b), (name, pair, p, "BGRA rule on the c8 picture")


@pytest.mark.parametrize("pair", PAIRS)
def test_the_clamp_at_zero_is_exercised_and_grey_stays_grey(host_tables, pair):
    lin = host_tables[pair][0].astype(np.int64)
    # saturated BT.2020 red: the green and blue rows of the primaries go negative
    a = np.array([lin[4095], 0, 0], np.int64)
    assert ((T.PRIMARIES @ a + 512) >> 10)[1:].max() < 0
    w, h = 64, 32
    y = np.sort(np.arange(w * h) % 1024).reshape(h, w)      # every ten-bit code, twice, in rising order
    for fmt in (T.P010, T.I010):
        Y, U, V = api.tonemap_frame(fmt, pair[0], pair[1], w, h, T.make_planes(fmt, y, np.full((h // 2, w // 2), 512), np.full((h // 2, w // 2), 512)), 0)
        assert np.all(U == 128) and np.all(V == 128)
        assert np.all(np.diff(Y.reshape(-1).astype(np.int64)) >= 0)      # Y does not decrease with Y'


@pytest.mark.parametrize("fmt", [T.P010, T.I010])
def test_the_bits_that_carry_no_value_are_ignored(fmt):
    w, h = 18, 10
    _, y, cb, cr = T.inputs(w, h)[0]
    junk = np.random.default_rng(3).integers(0, 64, (h, w))
    clean = api.tonemap_frame(fmt, T.HLG, 1000, w, h, T.make_planes(fmt, y, cb, cr), 1)
    dirty_planes = [T.make_planes(fmt, y, cb, cr, junk=junk)[0]] + T.make_planes(fmt, y, cb, cr, junk=63)[1:]
    dirty = api.tonemap_frame(fmt, T.HLG, 1000, w, h, dirty_planes, 1)
    assert all(np.array_equal(a, b) for a, b in zip(clean, dirty))


def test_refusals():
    lib = api.load_library()
    lib.vp8host_tonemap_tables.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.vp8host_tonemap_frame.argtypes = [C.c_int] * 6 + [C.c_void_p] * 6
    t = [np.empty(4096, np.uint32), np.empty(4096, np.uint32), np.empty(4096, np.uint8), np.empty(4096, np.uint8)]
    tp = [a.ctypes.data for a in t]
    assert lib.vp8host_tonemap_tables(T.PQ, 1000, *tp) == 0
    for transfer, peak in ((0, 1000), (3, 1000), (-1, 1000), (T.PQ, 399), (T.HLG, 10001), (T.PQ, 0)):
        assert lib.vp8host_tonemap_tables(transfer, peak, *tp) == -1, (transfer, peak)
    for k in range(4):
        assert lib.vp8host_tonemap_tables(T.PQ, 1000, *[None if i == k else p for i, p in enumerate(tp)]) == -1, k
    w, h = 18, 10
    src = np.zeros(w * h * 2, np.uint8)
    out = [np.empty(w * h, np.uint8) for _ in range(3)]
    ptrs = [src.ctypes.data] * 3 + [o.ctypes.data for o in out]
    assert lib.vp8host_tonemap_frame(T.P010, T.PQ, 1000, 0, w, h, *ptrs) == 0
    assert lib.vp8host_tonemap_frame(T.P010, T.PQ, 1000, 0, w, h, ptrs[0], ptrs[1], None, *ptrs[3:]) == 0      # P010 has no third plane
    for fmt in (0, 1, 6, 7, 16, 18, -1, 8):
        assert lib.vp8host_tonemap_frame(fmt, T.PQ, 1000, 0, w, h, *ptrs) == -1, fmt
    for transfer, peak, matrix, ww, hh in ((0, 1000, 0, w, h), (3, 1000, 0, w, h), (T.PQ, 399, 0, w, h), (T.PQ, 10001, 0, w, h), (T.PQ, 1000, 4, w, h),
                                           (T.PQ, 1000, -1, w, h), (T.PQ, 1000, 0, 17, h), (T.PQ, 1000, 0, w, 9), (T.PQ, 1000, 0, 0, h), (T.PQ, 1000, 0, w, -2)):
        assert lib.vp8host_tonemap_frame(T.I010, transfer, peak, matrix, ww, hh, *ptrs) == -1, (transfer, peak, matrix, ww, hh)
    for k in (0, 1, 2, 3, 4, 5):
        assert lib.vp8host_tonemap_frame(T.I010, T.PQ, 1000, 0, w, h, *[None if i == k else p for i, p in enumerate(ptrs)]) == -1, k
    for k in (0, 1, 3, 4, 5):
        assert lib.vp8host_tonemap_frame(T.P010, T.PQ, 1000, 0, w, h, *[None if i == k else p for i, p in enumerate(ptrs)]) == -1, k
