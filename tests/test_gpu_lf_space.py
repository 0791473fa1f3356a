"""The normal loop filter's three kernels -- k_loop_filter4 (what one context launches), k_loop_filter3_b (what every batch launches)
and k_loop_filter4_b (VP8HIP_LF_BATCH_FORM=4) -- and their vp8hip_conformant_stream instantiations against the CPU oracle, bit for
bit on Y, U and V: over the whole parameter space (tests/lf_cases.py: every level, five sharpness values, both tables of hev
thresholds, on contents at the ends of the ranges inside which lf_shared.h's rewritten edge arithmetic is exact -- what they reach is
asserted in test_lf_space_cpu.py), at the sizes around the band height (8 macroblock rows), the rings (8 and 16 macroblocks) and the
flush row, and with a level-0 macroblock ending the plane at chosen places in and between bands.

One context (or one batch of three) per test; between cases only the segment data and the reconstruction change, so successive
launches also walk the band-counter window.  VP8HIP_LF_BATCH_FORM is read once per process: k_loop_filter4_b runs the batch
functions of this file in a child process.  A filter that times out (VP8HIP_ERR_TIMEOUT from the bounded waits, or the child's time
limit) fails the test with what it has and launches nothing more.  Run with `pytest -m gpu`."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

if __name__ == "__main__":      # the child process: no conftest.py has set the path
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]

import numpy as np
import pytest

import lf_cases as lc
import lf_ref
from oracle_lib import Oracle
from test_lf_space_cpu import oracle_frame
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu

CONTENTS = list(lc.MAKERS)
MEMBERS = 3


@functools.lru_cache(maxsize=None)
def _content(name, mbw=lc.W // 16, mbh=lc.H // 16):
    return lc.Content(name, mbw, mbh)


@functools.lru_cache(maxsize=None)
def _oracle_mask(name, mbw=lc.W // 16, mbh=lc.H // 16):
    c = _content(name, mbw, mbh)
    nz, mask = np.zeros(len(c.seg), np.int32), np.zeros(len(c.seg), np.int32)
    Oracle.stages().prepare_filter_mask(c.coeffs.reshape(-1), nz, c.parts, mask, c.W, c.H)
    return mask


class Case:
    """one content under one table: what goes in, and what the oracle (the conformant one for conformant cases) makes of it"""

    def __init__(self, tag, c, sd, planes, conformant=False, seg=None):
        self.tag, self.c, self.sd, self.planes, self.conformant = tag + (" conformant" if conformant else ""), c, sd, planes, conformant
        self.seg = c.seg if seg is None else seg
        self.want = oracle_frame(planes, self.seg, c.mask, sd, conformant)


@functools.lru_cache(maxsize=None)
def sweep_case(name, k, conformant=False):
    tag, sd = lc.sweep()[k]
    c = _content(name)
    return Case(f"{name} {tag}", c, sd, c.planes(sd, k), conformant)


@functools.lru_cache(maxsize=None)
def geometry_case(name, mbw, mbh, table, conformant=False):
    levels, sharp = lc.GEOMETRY_TABLES[table]
    c = _content(name, mbw, mbh)
    return Case(f"{name} {mbw}x{mbh} levels {levels} sharpness {sharp}", c, lc.segments(levels, sharp), c.planes(), conformant)


def _compare(got, case, mask, what, bad):
    for name, g, w in zip("YUV", got, case.want):
        if not np.array_equal(g, w):
            d = np.argwhere(g != w)
            bad.append(f"{case.tag} {what}: {name} differs in {len(d)} samples, first (y, x) {d[:3].tolist()}")
    if mask is not None and not np.array_equal(mask, _oracle_mask(case.c.name, case.c.W // 16, case.c.H // 16)):
        bad.append(f"{case.tag} {what}: the filter mask differs")


# ---- form 4, one context --------------------------------------------------------------------------------------------------------
def single_differences(cases, launches=1):
    """[message] of the cases (one size) in which vp8hip_loop_filter and the oracle differ"""
    bad = []
    hip = api.Vp8Hip(cases[0].c.W, cases[0].c.H)
    try:
        loaded = None
        for case in cases:
            if loaded is not case.seg:
                hip.upload_mb_data(case.c.coeffs, case.c.parts, case.seg)
                loaded = case.seg
            hip.conformant_stream(case.conformant)
            hip.set_segments(case.sd)
            for l in range(launches):      # hand-off races show as launch-to-launch differences
                hip.upload_recon(*case.planes)
                hip.prepare_filter_mask(want_nz=False)
                hip.loop_filter()
                _compare(hip.download_last(), case, hip.debug(api.DBG_MB_MASK) if l == 0 else None, f"launch {l}", bad)
    except api.Vp8HipError as e:           # a timeout is a finding: stop here
        bad.append(f"stopped at {case.tag}: {e}")
    finally:
        hip.close()
    return bad


# ---- a batch of three: form 3, or k_loop_filter4_b in a process that reads VP8HIP_LF_BATCH_FORM=4 ----------------------------------
def batch_differences(rounds, launches=1):
    """rounds: [[Case] * MEMBERS], all of one size; each round is one vp8hip_batch_loop_filter (per launch) with a case per member"""
    bad = []
    lib = api.load_library()
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    lib.vp8hip_batch_loop_filter.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    c0 = rounds[0][0].c
    ctxs = [api.Vp8Hip(c0.W, c0.H) for _ in range(MEMBERS)]
    hb = C.c_void_p()
    try:
        for m in ctxs:
            m.set_segments(rounds[0][0].sd)
        assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * MEMBERS)(*[m.h for m in ctxs]), MEMBERS) == 0
        for cases in rounds:
            assert len(cases) == MEMBERS and len(set(c.conformant for c in cases)) == 1
            for i, (m, case) in enumerate(zip(ctxs, cases)):
                m.upload_mb_data(case.c.coeffs, case.c.parts, case.seg)
                m.conformant_stream(case.conformant)
                m.set_segments(case.sd)
            for l in range(launches):
                for m, case in zip(ctxs, cases):
                    m.upload_recon(*case.planes)
                    m.prepare_filter_mask(want_nz=False)
                rc = lib.vp8hip_batch_loop_filter(hb, None)
                if rc != 0:
                    raise api.Vp8HipError(f"vp8hip_batch_loop_filter: {rc}")
                for i, (m, case) in enumerate(zip(ctxs, cases)):
                    _compare(m.download_last(), case, m.debug(api.DBG_MB_MASK) if l == 0 else None, f"member {i} launch {l}", bad)
    except api.Vp8HipError as e:
        bad.append(f"stopped: {e}")
    finally:
        if hb:
            lib.vp8hip_batch_destroy(hb)
        for m in ctxs:
            m.close()
    return bad


def sweep_rounds(tables, contents=CONTENTS, conformant=False, rotate=True):
    """launch j: member m filters table tables[(j + 53 m) % n] -- every table in every member, the members of a launch on different
    tables -- on content (j + m) % len(contents): contents rotated over the members, not crossed with the tables.  rotate=False: member
    m stays on contents[m], which then meets every table."""
    n = len(tables)
    return [[sweep_case(contents[((j if rotate else 0) + m) % len(contents)], tables[(j + 53 * m) % n], conformant) for m in range(MEMBERS)]
            for j in range(n)]


CARRY_CONTENTS = ["clamps", "bounds", "clamps"]      # per member: the full sweep on clamps (and on bounds) in every batch form


def geometry_rounds(mbw, mbh):
    combos = [geometry_case(name, mbw, mbh, t) for name in ("lf_check", "bounds") for t in range(3)]
    rounds = [combos[0::2], combos[1::2]]       # each member of a round on its own table, both contents in it
    rounds.append([geometry_case("bounds", mbw, mbh, 1, True), geometry_case("bounds", mbw, mbh, 2, True), geometry_case("lf_check", mbw, mbh, 1, True)])
    return rounds


def level0_cases(conformant=False):
    """9 x 17 macroblocks, levels (6, 0, 14, 20): ONE macroblock of segment 1, which ends the plane there (CPU_kernels.cl:990), or none"""
    mbw, mbh = 9, 17
    c = _content("lf_check", mbw, mbh)
    sd = lc.segments((6, 0, 14, 20))
    base = np.where(c.seg == 1, 2, c.seg).astype(np.int32)
    out = []
    for stop in (0, 4, 7 * mbw + 8, 8 * mbw, 8 * mbw + 8, mbw * mbh - 1, None):
        seg = base.copy()
        if stop is not None:
            seg[stop] = 1
        case = Case(f"level 0 at macroblock {stop}", c, sd, c.planes(), conformant, seg=seg)
        case.stop = stop
        out.append(case)
    return out


def _check_level0_expectations(cases):
    """what the oracle says about the stop, so that the device's equality with it means what the issue asks: the rows below the
    stopping macroblock's row are untouched in all three planes, and something in front of it was filtered"""
    mbw = 9
    for case in cases:
        if case.stop is None:
            assert all((w[-8:] != p[-8:]).any() for w, p in zip(case.want, case.planes))
            continue
        row = case.stop // mbw
        for w, p, n in zip(case.want, case.planes, (16, 8, 8)):
            assert np.array_equal(w[(row + 1) * n:], p[(row + 1) * n:]), case.tag
            assert (w != p).any() == (case.stop > 0), case.tag      # (nothing at or behind the stop is filtered: what changed lies in front of it)


# ---- the tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONTENTS)
def test_form4_over_the_parameter_space(name):
    cases = [sweep_case(name, k) for k in range(len(lc.sweep()))]
    bad = single_differences(cases)
    assert not bad, f"{len(bad)} differences in {len(cases)} cases: {bad[:3]}"


def test_form3_batch_over_the_parameter_space():
    rounds = sweep_rounds(list(range(len(lc.sweep()))))
    bad = batch_differences(rounds)
    assert not bad, f"{len(bad)} differences in {len(rounds)} launches of {MEMBERS}: {bad[:3]}"


@pytest.mark.parametrize("name", ["bounds", "clamps"])
def test_form4_conformant_saturates_the_carry(name):
    """vp8hip_conformant_stream: the conformant oracle, which test_lf_space_cpu.py shows to be lf_ref.loop_filter(carry_saturates=True)
    on these very cases, and -- with it off again on the same context -- the reference's"""
    n = len(lc.sweep())
    cases = [sweep_case(name, k, conformant) for k in range(n) for conformant in (True, False)]
    assert any(not np.array_equal(a, b) for k in range(n) for a, b in zip(sweep_case(name, k, True).want, sweep_case(name, k).want))
    r = lf_ref.loop_filter(tuple(np.stack([sweep_case(name, k).planes[i] for k in range(n)]) for i in range(3)), cases[0].c.seg, cases[0].c.mask,
                           np.stack([sd for _, sd in lc.sweep()]), carry_saturates=True)
    assert all(np.array_equal(r.planes[i][k], sweep_case(name, k, True).want[i]) for k in range(n) for i in range(3))
    bad = single_differences(cases)
    assert not bad, f"{len(bad)} differences in {len(cases)} cases: {bad[:3]}"


def test_form3_batch_conformant_saturates_the_carry():
    tables = list(range(len(lc.sweep())))
    rounds = sweep_rounds(tables, CARRY_CONTENTS, True, rotate=False) + sweep_rounds(tables[::4], CARRY_CONTENTS, False, rotate=False)
    bad = batch_differences(rounds)
    assert not bad, f"{len(bad)} differences in {len(rounds)} launches of {MEMBERS}: {bad[:3]}"


@pytest.mark.parametrize("mbw,mbh", lc.GEOMETRIES)
def test_geometries_around_band_ring_and_flush_row(mbw, mbh):
    """form 4 alone and form 3 in a batch of three, three launches each, both carries; where the restatement takes no longer than the
    rest of the test it is asked as well"""
    rounds = geometry_rounds(mbw, mbh)
    if mbw * mbh <= 81:
        for case in rounds[2][:2]:
            r = lf_ref.loop_filter(case.planes, case.seg, case.c.mask, case.sd, carry_saturates=True)
            assert all(np.array_equal(g[0], w) for g, w in zip(r.planes, case.want)), case.tag
    bad = single_differences([case for cases in rounds for case in cases], launches=3)
    assert not bad, f"form 4: {len(bad)} differences: {bad[:3]}"
    bad = batch_differences(rounds, launches=3)
    assert not bad, f"form 3: {len(bad)} differences: {bad[:3]}"


def test_level_zero_ends_the_plane_at_a_chosen_macroblock():
    """first macroblock, middle of row 0, the last macroblock of a band, the first and last of the next band's first row, the very
    last, and not at all; in both modes (the plane-ending rule is the reference's in either)"""
    cases = level0_cases()
    _check_level0_expectations(cases)
    conformant = level0_cases(True)
    bad = single_differences(cases + conformant)
    assert not bad, f"form 4: {len(bad)} differences: {bad[:3]}"
    rounds = [[cases[0], cases[2], cases[6]], [cases[1], cases[3], cases[4]], [cases[6], cases[5], cases[2]],
              [conformant[3], conformant[6], conformant[5]]]
    bad = batch_differences(rounds, launches=2)
    assert not bad, f"form 3: {len(bad)} differences: {bad[:3]}"


# ---- k_loop_filter4_b and k_loop_filter4_b_conformant: the batch functions in a process that reads VP8HIP_LF_BATCH_FORM=4 -------------
def _child_plan(group):
    """[(rounds of one size, launches per round)]: a quarter of the tables with the contents rotated; the saturating carry on every
    table (clamps and bounds); every geometry; the level-0 stops"""
    tables = list(range(len(lc.sweep())))
    if group == "sweep":
        return [(sweep_rounds(tables[::4]), 1)]
    if group == "conformant":
        return [(sweep_rounds(tables, CARRY_CONTENTS, True, rotate=False), 1)]
    if group == "geometry":
        return [(geometry_rounds(mbw, mbh), 2) for mbw, mbh in lc.GEOMETRIES]
    cases, conformant = level0_cases(), level0_cases(True)
    return [([[cases[0], cases[2], cases[6]], [cases[1], cases[3], cases[4]], [cases[6], cases[5], cases[2]],
              [conformant[3], conformant[6], conformant[5]]], 1)]


def _child(group):
    bad, n = [], 0
    for rounds, launches in _child_plan(group):
        n += len(rounds)
        bad += batch_differences(rounds, launches)
        if any(b.startswith("stopped") for b in bad):      # a timeout: nothing further is launched
            break
    print(json.dumps({"form": os.environ.get("VP8HIP_LF_BATCH_FORM"), "rounds": n, "differences": bad[:20], "differing": len(bad)}))


@pytest.mark.parametrize("group", ["sweep", "conformant", "geometry", "level0"])
def test_form4_batch_in_a_child_process(group):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=dict(os.environ, VP8HIP_LF_BATCH_FORM="4"),
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the child did not finish in {e.timeout} s: {(e.stdout or b'')[-1000:]}")
    assert r.returncode == 0, f"exit {r.returncode}: " + r.stdout[-1000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"form"')][0])
    assert d["form"] == "4" and d["rounds"] == sum(len(rounds) for rounds, _ in _child_plan(group))
    assert d["differences"] == [] and d["differing"] == 0, d


if __name__ == "__main__":
    _child(sys.argv[1])
