"""What the normal loop filter's cases (tests/lf_cases.py) are and reach, on the CPU: the numpy restatement tests/lf_ref.py against
the oracle's vp8o_loop_filter_frame (the reference's carry) and against the RFC 6386 decoder's Decoder._loop_filter (the saturating
carry, level 0 skipping one macroblock), and the conditions the contents exist for.  test_gpu_lf_space.py runs the device on the
same cases.

Seeds (lf_cases.SEEDS: bounds 1, limits 10, clamps 13, lf_check 18) were taken from 1..59 as the first four whose segment maps
at 9 x 9 macroblocks show segments 0, 1 and 2 before the first macroblock of segment 3 -- the sweep puts its level 0 there, so the
table that has it filters with its other three levels before the plane ends; the reach conditions below held for them as drawn."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import lf_cases as lc
import lf_ref
from oracle_lib import Oracle
from vp8_decode import Decoder

CONTENTS = list(lc.MAKERS)


@functools.lru_cache(maxsize=None)
def sweep_inputs(name):
    """(content, per-case planes, the three stacked planes, stacked segment data) of the sweep on content `name`"""
    cases = lc.sweep()
    c = lc.Content(name)
    per_case = [c.planes(sd, k) for k, (_, sd) in enumerate(cases)]
    stacked = tuple(np.stack([p[i] for p in per_case]) for i in range(3))
    return c, per_case, stacked, np.stack([sd for _, sd in cases])


@functools.lru_cache(maxsize=None)
def restated(name, carry_saturates=False, level0_ends_plane=True):
    c, _, stacked, sds = sweep_inputs(name)
    return lf_ref.loop_filter(stacked, c.seg, c.mask, sds, carry_saturates, level0_ends_plane, count=not carry_saturates)


def oracle_frame(planes, seg, mask, sd, conformant=False):
    """vp8o_loop_filter_frame on copies of the three planes"""
    st = Oracle.stages()
    out = []
    Oracle.lib().vp8o_set_conformant_stream(int(conformant))
    try:
        for p, n in zip(planes, (16, 8, 8)):
            f = np.ascontiguousarray(p).copy()
            st.loop_filter_frame(f, np.ascontiguousarray(seg, np.int32), np.ascontiguousarray(mask, np.int32),
                                 np.ascontiguousarray(sd, np.int32).reshape(-1), f.shape[1], f.shape[0], n)
            out.append(f)
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)
    return out


def _against_oracle(name, conformant):
    c, per_case, _, _ = sweep_inputs(name)
    r = restated(name, carry_saturates=conformant)
    bad = []
    for k, (tag, sd) in enumerate(lc.sweep()):
        for i, f in enumerate(oracle_frame(per_case[k], c.seg, c.mask, sd, conformant)):
            if not np.array_equal(f, r.planes[i][k]):
                bad.append(f"{tag} plane {'YUV'[i]}: {int((f != r.planes[i][k]).sum())} samples")
    assert not bad, f"{len(bad)} planes differ: {bad[:3]}"


@pytest.mark.parametrize("name", CONTENTS)
def test_restatement_is_the_oracle(name):
    _against_oracle(name, False)
    assert (restated(name).planes[0] != sweep_inputs(name)[2][0]).any()


@pytest.mark.parametrize("name", CONTENTS)
def test_restatement_with_saturating_carry_is_the_conformant_oracle(name):
    _against_oracle(name, True)


@pytest.mark.parametrize("name", CONTENTS)
def test_restatement_in_decoder_mode_is_the_decoder(name):
    """carry_saturates and level 0 skipping the macroblock alone: RFC 6386 as tests/vp8_decode.py restates it, which derives the
    limits from level, sharpness and frame type itself -- so lf_cases.segments' tables are checked with it"""
    c, per_case, _, _ = sweep_inputs(name)
    r = restated(name, True, False)
    dec = Decoder()
    bad = []
    for k, (levels, sharp, key) in enumerate(lc.sweep_parameters()):
        f = SimpleNamespace(mbw=c.W // 16, mbh=c.H // 16, segmentation_enabled=True, segment_id=c.seg, seg_lf=list(levels), seg_abs=True,
                            loop_filter_level=0, sharpness=sharp, key=key)
        planes = [p.copy() for p in per_case[k]]
        dec._loop_filter(f, planes, c.mask == 0)
        for i in range(3):
            if not np.array_equal(planes[i], r.planes[i][k]):
                bad.append(f"{lc.sweep()[k][0]} plane {'YUV'[i]}")
    assert not bad, f"{len(bad)} planes differ: {bad[:3]}"


def test_sweep_holds_every_level_sharpness_and_both_threshold_tables():
    p = lc.sweep_parameters()
    assert len(p) == 160
    for key in (False, True):
        for sharp in lc.SHARPNESS:
            levels = sorted(l for lv, s, k in p if s == sharp and k == key for l in lv)
            assert levels == list(range(64))
    assert all(min(lv) < 16 and max(lv) >= 48 for lv, _, _ in p)
    sds = np.stack([sd for _, sd in lc.sweep()])
    assert set(sds[:, :, 10].ravel()) == {0, 1, 2, 3}
    assert sds[:, :, 9].min() == 1 and sds[:, :, 9].max() == 63 and (sds[:, :, 9] < sds[:, :, 6]).any()   # interior limits below the level
    # the default table of every earlier test is what it was
    assert lc.segments((6, 10, 14, 20))[:, 6:].tolist() == [[6, 22, 18, 6, 0], [10, 34, 30, 10, 0], [14, 46, 42, 14, 0], [20, 64, 60, 20, 2]]


def test_filter_mask_is_the_oracles():
    c = lc.Content("lf_check")
    nz, mask = np.zeros(len(c.seg), np.int32), np.zeros(len(c.seg), np.int32)
    Oracle.stages().prepare_filter_mask(c.coeffs.reshape(-1), nz, c.parts, mask, c.W, c.H)
    assert np.array_equal(mask, c.mask)
    y2_only = (np.abs(c.coeffs[:, :24]).sum(axis=(1, 2)) == 0) & (c.coeffs[:, 24, 0] != 0)
    assert (y2_only & (c.parts == 0) & (c.mask != 0)).any() and (y2_only & (c.parts != 0)).any()   # the Y2 DC counts for a whole macroblock


@pytest.mark.parametrize("name", ["limits", "clamps"])
def test_reach_of_the_limit_and_clamp_contents(name):
    """Conditions, not measurements: over the sweep, macroblock edges and inner edges each meet every test exactly at its limit and one
    past it, both clamps at both ends while the mask passes, the range the kernels' `123` stands for, and a carried register out of
    range at both ends.  (All of them are reachable: none had to be dropped.  The first clamp needs |p1-p0| and |q1-q0| near an
    interior limit of 50 or more and all three steps pointing one way, which only clamps' profiles draw; limits carries two
    macroblock columns of them.)"""
    reach = restated(name).reach
    missing = [(kind, n) for kind in lf_ref.KINDS for n in lf_ref.NAMES if reach.total(kind, n) == 0]
    assert not missing, missing
    r, s = restated(name), restated(name, True)
    assert any((r.planes[i] != s.planes[i]).any() for i in range(3)), "the two carry disciplines never differ on this content"


def test_bounds_makes_the_two_carries_differ_in_luma_and_in_chroma():
    r, s = restated("bounds"), restated("bounds", True)
    cases = [int((r.planes[i] != s.planes[i]).any(axis=(1, 2)).sum()) for i in range(3)]
    assert cases[0] > 0 and cases[1] + cases[2] > 0, cases


@pytest.mark.parametrize("name", CONTENTS)
def test_every_level_of_every_table_is_used(name):
    """each non-zero level by a macroblock that is filtered; level 0 (one table per sharpness and frame type) by the macroblock that
    ends the plane behind macroblocks of the three other segments"""
    c = sweep_inputs(name)[0]
    filtered = restated(name).filtered
    for k, (levels, _, _) in enumerate(lc.sweep_parameters()):
        for s, level in enumerate(levels):
            used = filtered[k] & (c.seg == s)
            if level:
                assert used.any(), (name, levels, s)
            else:
                stop = int(np.argmax(c.seg == s))
                assert not filtered[k, stop:].any() and set(c.seg[:stop]) == {0, 1, 2, 3} - {s}, (name, levels, stop)


def test_the_measured_rarity_of_the_unsaturated_carry():
    """REFERENCE_DEFECTS.md's figure: 64x48 luma, every level 63, sharpness 0, inter thresholds, content within 40 of 0, random
    segments, seeds 0..39 -- the reference's filter (the oracle) and a decoder's (Decoder._loop_filter) part ways in a few dozen
    samples (26, in 16 of the 40 seeds, by up to 4), and the clamp at the hand-over removes every one of them"""
    sd = lc.segments((63, 63, 63, 63))
    dec, total, seeds_hit, worst = Decoder(), 0, 0, 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        y = np.clip(rng.integers(-40, 41, size=(48, 64)) * (rng.random((48, 64)) < 0.5), 0, 255).astype(np.uint8)
        seg = rng.integers(0, 4, size=12).astype(np.int32)
        mask = np.where(rng.random(12) < 0.8, -1, 0).astype(np.int32)
        u = np.zeros((24, 32), np.uint8)
        o = oracle_frame((y, u, u), seg, mask, sd)[0]
        f = SimpleNamespace(mbw=4, mbh=3, segmentation_enabled=True, segment_id=seg, seg_lf=[63] * 4, seg_abs=True, loop_filter_level=0,
                            sharpness=0, key=False)
        planes = [y.copy(), u.copy(), u.copy()]
        dec._loop_filter(f, planes, mask == 0)
        assert np.array_equal(oracle_frame((y, u, u), seg, mask, sd, conformant=True)[0], planes[0]), f"seed {seed}: the clamped carry is not the whole cause"
        assert np.array_equal(lf_ref.loop_filter((y, u, u), seg, mask, sd).planes[0][0], o)
        n = int((o != planes[0]).sum())
        total, seeds_hit, worst = total + n, seeds_hit + (n > 0), max(worst, int(np.abs(o.astype(int) - planes[0]).max()))
    print(f"unsaturated carry: {total} samples differ over 40 seeds of 64x48 ({seeds_hit} seeds show any), largest difference {worst}")
    assert total > 0 and seeds_hit < 40


# ---- the geometry cases of test_gpu_lf_space.py ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry_expected(name, mbw, mbh, table, conformant):
    """(content, [Y, U, V]) by the oracle"""
    c = lc.Content(name, mbw, mbh)
    levels, sharp = lc.GEOMETRY_TABLES[table]
    return c, oracle_frame(c.planes(), c.seg, c.mask, lc.segments(levels, sharp), conformant)


def test_geometry_cases_on_bounds_separate_the_two_carries_and_the_restatement_agrees():
    """test_gpu_lf_space.py holds the conformant kernels to the conformant oracle at these sizes: here the restatement says the same
    (the sizes whose restatement takes a second or less), and the two oracles differ at most of the sizes -- neither device assertion
    can pass by coincidence"""
    differ = {}
    for mbw, mbh in lc.GEOMETRIES:
        for t in (1, 2):
            c, ref = geometry_expected("bounds", mbw, mbh, t, False)
            _, con = geometry_expected("bounds", mbw, mbh, t, True)
            differ[(mbw, mbh)] = differ.get((mbw, mbh), 0) + sum(int((a != b).sum()) for a, b in zip(ref, con))
            if mbw * mbh <= 81:
                levels, sharp = lc.GEOMETRY_TABLES[t]
                for cs, want in ((False, ref), (True, con)):
                    got = lf_ref.loop_filter(c.planes(), c.seg, c.mask, lc.segments(levels, sharp), carry_saturates=cs).planes
                    assert all(np.array_equal(g[0], w) for g, w in zip(got, want)), (mbw, mbh, t, cs)
    assert differ[(33, 17)] > 0 and differ[(9, 9)] > 0 and sum(v > 0 for v in differ.values()) >= 8, differ
