"""The parallel boolean coder (k_ent_maps, k_ent_walk, k_ent_encode, k_ent_finish) on bool strings of the tests' own making
(vp8hip_debug_bool_code), byte-exact against the oracle's serial coder: carry ladders placed in every lane / wave / step relation
k_ent_finish distinguishes, the seams of chunks, super-chunks and partitions, and words that take many adds.  Coefficient data
reaches none of the carry cases (a pre-carry word is 0xffffffff once in 2^32) and the seams only by luck.  What each string is
there for is asserted from the exact model in tests/test_bool_coder_cpu.py."""
import numpy as np
import pytest

import bool_coder_ref as R
from entropy_cases import synthetic
from oracle_lib import oracle_bool_code
from pipeline import default_segments
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu

LADDERS = [(name, carried) for name in R.PLACEMENTS for carried in (True, False)]
LADDER_IDS = [f"{n}-{'carried' if c else 'standing'}" for n, c in LADDERS]
FILL = 0xa5


@pytest.fixture(scope="module")
def hip():
    h = api.Vp8Hip(128, 128)       # 102 400 bools of coder scratch
    yield h
    h.close()


_expected = {}


def expected(b) -> bytes:
    key = b.tobytes()
    if key not in _expected:
        _expected[key] = oracle_bool_code(b)
    return _expected[key]


def check(hip, strings, tag):
    """partitions and sizes as the serial coder's; nothing written between a partition's end and the next partition's start"""
    exp = [expected(b) for b in strings]
    step = max(len(e) for e in exp) + 24
    out = np.full(len(strings) * step, FILL, np.uint8)
    got = hip.debug_bool_code(strings, step, out)
    for p, (g, e) in enumerate(zip(got, exp)):
        assert len(g) == len(e), f"{tag}: partition {p} is {len(g)} bytes, the serial coder's {len(e)}"
        if g != e:
            bad = np.nonzero(np.frombuffer(g, np.uint8) != np.frombuffer(e, np.uint8))[0]
            raise AssertionError(f"{tag}: partition {p} ({len(strings[p])} bools, {len(e)} bytes) differs at bytes {bad[:8]} "
                                 f"({len(bad)} in all): {g[bad[0]:bad[0] + 8].hex()} for {e[bad[0]:bad[0] + 8].hex()}")
        rest = out[p * step + len(e):(p + 1) * step]
        assert np.all(rest == FILL), f"{tag}: partition {p}: bytes behind its end were written"


@pytest.mark.parametrize("name,carried", LADDERS, ids=LADDER_IDS)
def test_carry_ladder(hip, name, carried):
    check(hip, [R.placement(name, carried)], name)


@pytest.mark.parametrize("name", list(R.PLACEMENTS))
def test_carry_ladder_as_a_later_partition(hip, name):
    """word_base is not 0; random and empty neighbours"""
    up, down = R.placement(name, True), R.placement(name, False)
    r = lambda n: R.random_bools(50 + n, n)
    e = r(0)
    check(hip, [r(513), up, e], name + " P3 carried")
    check(hip, [e, r(2049), down], name + " P3 standing")
    check(hip, [r(255), e, up, r(2049), e, r(33), down, e], name + " P8")
    check(hip, [e, e, e, e, e, e, e, up], name + " P8 last")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_seams_one_partition(hip, family):
    for b in R.seam_strings(family):
        check(hip, [b], f"{family} {len(b)}")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_seams_partitions(hip, family):
    for name, parts in R.seam_partitions(family):
        check(hip, parts, f"{family} {name}")


def test_dense_adds(hip):
    dense, ones, mixed = R.dense_string(), R.pure_dense("ones"), R.pure_dense("mixed")
    for b, tag in ((dense, "dense"), (ones, "ones"), (mixed, "mixed")):
        check(hip, [b], tag)
    check(hip, [ones, dense[:40000], mixed], "dense P3")


def test_the_tap_leaves_the_context_as_it_was():
    """count_probs / encode_coefficients give the same bytes before and after tap calls, one of them longer than the scratch"""
    mbw = mbh = 8
    coeffs, parts, nz = synthetic(mbw, mbh, 11)
    h = api.Vp8Hip(mbw * 16, mbh * 16)
    try:
        h.set_segments(default_segments())
        h.upload_mb_data(coeffs, parts, np.zeros(mbw * mbh, np.int32))
        h.prepare_filter_mask()
        probs, denom = h.count_probs(4)
        before = h.encode_coefficients(probs, 4)
        check(h, [R.random_bools(7, 3000), R.random_bools(8, 0), R.placement("whole_wave", True)], "tap between")
        after = h.encode_coefficients(probs, 4)            # (no count_probs in between: the tap has not touched what it left)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        check(h, [R.random_bools(9, 150000)], "longer than the scratch")      # 102 400 bools: the scratch grows
        probs2, denom2 = h.count_probs(4)
        assert np.array_equal(probs, probs2) and np.array_equal(denom, denom2)
        again = h.encode_coefficients(probs2, 4)
        assert all(np.array_equal(a, b) for a, b in zip(before, again))
    finally:
        h.close()


def test_the_tap_refuses_what_it_cannot_code(hip):
    ok = R.random_bools(3, 100)
    bad = ok.copy()
    bad[50] &= 0xff00                                           # probability 0
    for strings in ([bad], [ok, bad], [], [ok] * 9):
        with pytest.raises(api.Vp8HipError):
            hip.debug_bool_code(strings, 4096)
    two_bits = ok.copy()
    two_bits[3] |= 0x200
    with pytest.raises(api.Vp8HipError):
        hip.debug_bool_code([two_bits], 4096)
    with pytest.raises(api.Vp8HipError, match="-7"):            # VP8HIP_ERR_OVERFLOW: a partition longer than partition_step
        hip.debug_bool_code([R.random_bools(4, 4096)], 64)
    with pytest.raises(api.Vp8HipError, match="-7"):            # ... and more bools than the scratch at its largest (304 per block) holds
        hip.debug_bool_code([np.full(1600 * 304 + 1, 128, np.uint16)], 1 << 20)
    check(hip, [ok], "after the refusals")
