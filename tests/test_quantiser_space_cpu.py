"""The macroblock stage of the restatement (oracle/vp8_oracle.c) over the whole quantiser space -- every index 0..127, the index deltas at
both ends of qi()'s clamp, ladders of indices under the SSIM targets that stop the segment loop at every pass -- on content that takes
the coefficients to the bounds the device code's narrow arithmetic is justified by (tests/quantiser_cases.py):
  (1) what the content reaches, asserted on the restatement alone (runs everywhere);
  (2) the restatement against the reference's own kernels compiled for x86, live, on the same cases (only where oracle/_ref was built).
Bit-exact for every integer output; MB_SSIM (float in the reference) within 1e-4; block 24 where it exists (16x16 macroblocks).

Reached by these cases (printed by the first test): |Y2 DC| 2040 with both signs (the numerator 16320 of tdiv's comment over y2dc = 8),
|Y2 AC| 1020, split-macroblock luma DC 510 and chroma DC 510 (2040 over the smallest first-order quantiser), first-order AC 316 (luma)
and 314 (chroma), MB_parts 0 and 1."""
import numpy as np
import pytest

import quantiser_cases as qc
from pipeline import run_inter_frame

SSIM_TOL = 1e-4
PAIRS = qc.cpu_case_list()


def test_the_cases_reach_the_bounds_the_device_arithmetic_is_justified_by():
    rows = {n: qc.reach([p for p in PAIRS if p[0] == n]) for n in qc.CONTENTS}
    cols = ("y2_dc_min", "y2_dc_max", "y2_ac", "split_luma_dc", "ac", "chroma_ac", "chroma_dc")
    print("\n%-18s" % "content" + "".join("%14s" % c for c in cols) + "  parts  recon has 0 and 255")
    for n, r in rows.items():
        print("%-18s" % n + "".join("%14d" % r[c] for c in cols) + f"  {sorted(r['parts'])}  {r['recon_0_and_255']}")
    allr = qc.reach(PAIRS)
    assert allr["y2_dc_max"] == 2040 and allr["y2_dc_min"] == -2040, (allr["y2_dc_min"], allr["y2_dc_max"])
    assert rows["flat_up"]["y2_dc_max"] == 2040 and rows["flat_down"]["y2_dc_min"] == -2040
    assert allr["y2_ac"] >= 1020, allr["y2_ac"]
    assert allr["chroma_dc"] == 510, allr["chroma_dc"]
    assert allr["split_luma_dc"] == 510, allr["split_luma_dc"]
    assert allr["ac"] >= 250 and allr["chroma_ac"] >= 250, (allr["ac"], allr["chroma_ac"])
    assert 0 in allr["parts"] and len(allr["parts"]) > 1, allr["parts"]
    assert allr["recon_0_and_255"]
    assert allr["max_coefficient"] >= 1091        # a DCT_CAT6 token with its top extra bit set (the entropy stage on these frames)


def test_the_ladders_reach_every_exit_of_the_segment_loop():
    hist = {}
    for t in qc.TARGETS:
        hist[t] = qc.reach([(n, c) for n in qc.LOOP_CONTENTS for c in qc.ladders((t,))])["segments"]
        print(f"target {t}: macroblocks per segment {hist[t].tolist()}")
    total = len(qc.LOOP_CONTENTS) * len(qc.LADDERS) * 12
    assert (hist[0.90] > 0).all() and (hist[0.97] > 0).all(), hist
    assert hist[2.0].tolist() == [total, 0, 0, 0], hist[2.0]       # all four passes ran, the last one counts
    assert hist[0.5].tolist() == [0, 0, 0, total], hist[0.5]       # one pass


def test_only_segment_zeros_deltas_are_read():
    """the junk deltas of segments 1-3 change nothing: the same case without them gives the same coefficients"""
    for n in ("squares_inv", "hadamard"):
        for tag, sd, target in qc.delta_sets()[::9] + qc.ladders((0.97,)):
            clean = sd.copy()
            clean[1:, 1:6] = 0
            a = qc.restatement(n, (tag, sd, target))
            b = qc.restatement(n, (tag + "_clean", clean, target))
            assert np.array_equal(a["MB_coeffs"], b["MB_coeffs"]) and np.array_equal(a["recon_Y"], b["recon_Y"]), (n, tag)


def test_the_reciprocal_rule_of_the_device_division_restated():
    """tdiv (kernels_mb.hip): n / q as the high half of n * ((2^24 / q + 1) << 8).  Exact for every n < 2^15 and 2 <= q < 512, as its
    comment says; the first wrong quotient over all q is n = 34035 at q = 508, about twice the largest numerator there is (16320).
    This is the rule in numpy, not the device code: that is held by test_gpu_quantiser_space.py."""
    n = np.arange(1 << 16, dtype=np.uint64)
    first = (1 << 16, 0)
    for q in range(2, 512):
        wrong = np.nonzero((n * np.uint64(((1 << 24) // q + 1) << 8)) >> np.uint64(32) != n // np.uint64(q))[0]
        if wrong.size:
            first = min(first, (int(wrong[0]), q))
    assert first == (34035, 508), first


def _diff(a, b):
    bad = []
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, list):
            bad += [(k, i) for i, (x, y) in enumerate(zip(va, vb)) if not np.array_equal(x, y)]
        elif va.dtype == np.float32:
            if float(np.abs(va - vb).max()) > SSIM_TOL:
                bad.append((k, float(np.abs(va - vb).max())))
        elif k == "MB_coeffs":      # block 24 exists only for 16x16 macroblocks
            x, y = va.copy(), vb.copy()
            x[a["MB_parts"] != 0, 24] = 0
            y[b["MB_parts"] != 0, 24] = 0
            if not np.array_equal(x, y):
                bad.append((k, int((x != y).sum())))
        elif not np.array_equal(va, vb):
            bad.append((k, int((va != vb).sum())))
    return bad


@pytest.mark.parametrize("name", list(qc.CONTENTS))
def test_restatement_matches_reference_kernels_live_over_the_quantiser_space(name, reference_stages):
    cur, refs, (ug, ua) = qc.CONTENTS[name]
    bad = []
    cases = [c for n, c in PAIRS if n == name]
    for case in cases:
        tag, sd, target = case
        d = _diff(qc.restatement(name, case), run_inter_frame(reference_stages, cur, refs, sd, ug, ua, target))
        if d:
            bad.append((tag, d))
    assert not bad, f"{name}: restatement differs from the reference's kernels in {len(bad)} of {len(cases)} cases: {bad[:4]}"
