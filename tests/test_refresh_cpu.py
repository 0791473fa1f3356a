"""Cyclic intra refresh without a GPU: vp8host_intra_refresh_forced / _count against the Python restatement of include/vp8hip_host.h's
rule (tests/refresh_ref.py) for every period 4 .. 64 and every phase below two periods on grids from 1x1 to 13x12; the two properties
the multiplier 2 is there for (independence, coverage); every refusal; and the host first-partition coder on a frame with the rule's
is_inter, read back by tests/vp8_parse.py.  Everything is exact.  The tests of the entry points fail on a tree without the feature (the
entry points do not exist); the decoder test checks the expectation itself -- the test reference and nothing of the library -- and passes
on any tree.  tests/test_gpu_refresh.py holds the kernel and the native driver to the same restatement."""
import ctypes as C

import numpy as np
import pytest

import refresh_ref as ref
from vp8oclenc_amd import api

MBW, MBH = 13, 12
PERIODS = range(4, 65)


def host_map(period, q, mbw=MBW, mbh=MBH):
    return np.array([[api.intra_refresh_forced(period, q, r, c) for c in range(mbw)] for r in range(mbh)], bool)


@pytest.mark.parametrize("period", [4, 5, 7, 8, 13, 30, 64])
def test_the_predicate_equals_the_rule_macroblock_by_macroblock(period):
    for q in range(2 * period):
        assert np.array_equal(host_map(period, q), ref.forced_map(MBW, MBH, period, q)), (period, q)


def test_the_count_equals_the_sum_of_the_predicate_on_every_grid():
    """every period 4 .. 64, every q < 2 P, every grid 1x1 .. 13x12: the count against the rule's sum (a summed-area table of the rule's
    13x12 map gives all 156 grids), and for a sample against the sum of the HOST predicate"""
    lib = api.load_library()
    lib.vp8host_intra_refresh_count.argtypes = [C.c_int] * 4
    for period in PERIODS:
        for q in range(2 * period):
            table = ref.forced_map(MBW, MBH, period, q).astype(np.int64).cumsum(0).cumsum(1)
            got = np.array([[lib.vp8host_intra_refresh_count(w, h, period, q) for w in range(1, MBW + 1)] for h in range(1, MBH + 1)])
            assert np.array_equal(got, table), (period, q)
    for period, q, w, h in ((4, 3, 13, 12), (5, 9, 7, 3), (30, 41, 11, 9), (64, 100, 13, 12), (4, 0, 1, 1), (7, 13, 2, 5)):
        assert api.intra_refresh_count(w, h, period, q) == int(host_map(period, q, w, h).sum())


@pytest.mark.parametrize("period", PERIODS)
def test_independence_and_coverage(period):
    """no forced macroblock has a forced left, above, above-left or above-right neighbour; every macroblock is forced exactly once in
    any P consecutive phases"""
    maps = [ref.forced_map(MBW, MBH, period, q) for q in range(2 * period)]
    for q, m in enumerate(maps):
        p = np.zeros((MBH + 1, MBW + 2), bool)
        p[1:, 1:-1] = m
        for dr, dc in ((0, -1), (-1, 0), (-1, -1), (-1, 1)):
            assert not (m & p[1 + dr:1 + dr + MBH, 1 + dc:1 + dc + MBW]).any(), (period, q, dr, dc)
    for start in (0, 1, period - 1, period):
        assert (sum(m.astype(int) for m in maps[start:start + period]) == 1).all(), (period, start)
    # ... and the host function says the same at the two ends of the phase range
    for q in (0, 2 * period - 1):
        assert np.array_equal(host_map(period, q), maps[q])


def test_refusals():
    lib = api.load_library()
    lib.vp8host_intra_refresh_forced.argtypes = [C.c_int] * 4
    lib.vp8host_intra_refresh_count.argtypes = [C.c_int] * 4
    for period in (0, 1, 2, 3, 1025, 4096, -4):
        assert lib.vp8host_intra_refresh_forced(period, 0, 0, 0) == -1, period
        assert lib.vp8host_intra_refresh_count(4, 4, period, 0) == -1, period
        with pytest.raises(ValueError):
            api.intra_refresh_forced(period, 0, 0, 0)
        with pytest.raises(ValueError):
            api.intra_refresh_count(4, 4, period, 0)
    for period in (4, 1024):
        assert lib.vp8host_intra_refresh_forced(period, 0, 0, 0) == 1 and lib.vp8host_intra_refresh_forced(period, 1, 0, 0) == 0
        assert lib.vp8host_intra_refresh_count(1, 1, period, 0) == 1
    for q, r, c in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert lib.vp8host_intra_refresh_forced(4, q, r, c) == -1
    for w, h, q in ((0, 4, 0), (4, 0, 0), (4, 4, -1)):
        assert lib.vp8host_intra_refresh_count(w, h, 4, q) == -1
    # large phases and rows: no overflow on the way to the remainder
    assert lib.vp8host_intra_refresh_forced(1024, 2 ** 31 - 1, 2 ** 30, 5) == int((5 + 2 * 2 ** 30) % 1024 == (2 ** 31 - 1) % 1024)


@pytest.mark.parametrize("mbw,mbh,period,q", [(4, 3, 4, 0), (13, 12, 4, 3), (13, 12, 7, 9), (11, 9, 30, 17), (5, 2, 5, 4)])
def test_the_host_header_coder_writes_exactly_the_rules_macroblocks_as_intra(mbw, mbh, period, q):
    """a random inter frame whose is_inter is the rule's, through vp8bs_encode_header and back through the
    RFC 6386 parser: the intra macroblocks are the rule's, B_PRED with TM_PRED chroma, and the inter ones keep their references"""
    import vp8_parse as vp
    from bitstream_cases import default_sd, random_inter_case
    from vp8oclenc_amd import bitstream
    W, H = 16 * mbw, 16 * mbh
    fm = ref.forced_map(mbw, mbh, period, q).reshape(-1)
    case = random_inter_case(mbw, mbh, seed=period * 100 + q, long_mv=0.0)      # (vectors a search can find: within the frame's reach)
    case["is_inter"] = (~fm).astype(np.int32)
    case["replaced"] = int(fm.sum())
    assert case["replaced"] == api.intra_refresh_count(mbw, mbh, period, q) > 0
    hdr, _ = bitstream.encode_header(W, H, (0, 0, 0), default_sd(), case["seg"], case["nz"], case["probs"], case["denom"], case["skip_prob"],
                                     ref_frame=case["ref_frame"], parts=case["parts"], vectors=case["vectors"], is_inter=case["is_inter"],
                                     modes=case["modes"], replaced=case["replaced"])
    st = vp.StreamState()
    st.width, st.height = W, H      # (what a key frame would have set)
    f = vp.parse_frame(bitstream.gather_frame(hdr, [np.zeros(4096, np.uint8)]).tobytes(), st)
    assert not f.key and f.first_partition_overrun == 0
    assert np.array_equal(f.is_inter == 0, fm)
    assert (f.ymode[fm] == vp.B_PRED).all() and (f.uvmode[fm] == vp.TM_PRED).all()
    assert np.array_equal(f.ref_frame[~fm], case["ref_frame"][~fm] + 1) and (f.ref_frame[fm] == 0).all()
    assert np.array_equal(f.segment_id, case["seg"])


@pytest.mark.parametrize("layers", [1, 2])
def test_an_oracle_refresh_sequence_decodes_to_its_reconstruction_and_covers_the_picture(layers):
    """the expectation tests/test_gpu_refresh.py uses, judged by a decoder that shares no code with it: the CPU oracle's frame loop with
    the rule at P = 4 (conformant stream), every frame decoded: the decoded picture is the loop's reconstruction, the parsed intra set
    is the rule's at the loop's phase, the phase counts LAST-refreshing frames only, and P such frames cover the picture"""
    import arf_ref
    import temporal_ref
    import vp8_decode
    w, h, total, P = 64, 48, 10, 4
    mbw, mbh = w // 16, h // 16
    frames = arf_ref.noisy_pan(w, h, total, seed=w + total)
    recs = ref.oracle_loop(frames, layers, lambda t: P, conformant=True, gop_size=total, altref_range=total + 1, qi_min=10, qi_max=60)
    assert [r["key"] for r in recs] == [t == 0 for t in range(total)]
    dec = vp8_decode.Decoder()
    q, sets = 0, []
    for r in recs:
        f, planes = dec.decode(temporal_ref.record_bytes(r, w, h, 1))
        for name, g, want in zip("YUV", planes, r["recon"]):
            assert np.array_equal(g, want), (r["t"], name)
        if r["key"]:
            continue
        last = r["layer"]["refresh"] == temporal_ref.LAST
        want = ref.forced_map(mbw, mbh, P, q).reshape(-1) if last else np.zeros(mbw * mbh, bool)
        assert r["refresh"]["q"] == q and r["refresh"]["forced"] == int(want.sum()), r["t"]
        assert np.array_equal(f.is_inter == 0, want), r["t"]
        if last:
            sets.append(want)
            q += 1
    assert len(sets) >= P and all(np.logical_or.reduce(sets[i:i + P]).all() for i in range(len(sets) - P + 1))


def test_the_library_exports_the_entry_points():
    lib = api.load_library()
    for name in ("vp8host_intra_refresh_forced", "vp8host_intra_refresh_count", "vp8hip_intra_refresh", "vp8drv_set_intra_refresh", "vp8drv_get_intra_refresh"):
        assert hasattr(lib, name) and name in api.ABI_SYMBOLS, name
