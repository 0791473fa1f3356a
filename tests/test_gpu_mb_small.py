"""The macroblock kernels (kernels_mb.hip) on the smallest frames at which their workgroup structure can go wrong, against the CPU oracle
through the C ABI, bit for bit -- coefficients, block 24, MB_SSIM by its bit pattern, the non-zero counts and the filter mask, the
reconstruction before and after the loop filter.  A workgroup takes eight macroblocks:
    16x16     one macroblock and seven dead slots;
    48x32     six: one partial workgroup;
    144x16    nine: two workgroups, the second with one macroblock.
The content (mixed, below) is made so that the frame holds split and unsplit macroblocks and winners in all three references (asserted on
the oracle's own results over the three sizes); it runs at quantiser indices 0 and 127 and under ONE SSIM target on a ladder of indices, at
which macroblocks leave the segment loop after one, two and four passes (asserted likewise).  flat_up / flat_down of quantiser_cases.py at
index 0 take the second-order DC to +2040 and -2040, the largest numerator the signed division meets.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import quantiser_cases as qc
from oracle_lib import Oracle
from test_gpu_parity import _compare
from test_gpu_quantiser_space import KEYS, _frame
from test_gpu_search_saturating import _binary, _prepare
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (48, 32), (144, 16)]
TARGET = 0.98                                   # the one SSIM target of the ladder
LADDER = (30, 70, 100, 127)                      # segment 3 (the first pass) is the coarsest


def mixed(W, H):
    """[LAST, GOLDEN, ALTREF sources, current]: three frames of random 4-pixel squares, and a current frame whose macroblock m is macroblock
    m of reference m % 3 -- whole, or (every other macroblock) its four 8x8 quadrants taken from places one and two pixels apart, which makes
    the macroblock split -- with single pixels inverted at a density that grows with m, so that the residual, and with it the pass at which
    a macroblock meets the target, differs from macroblock to macroblock"""
    rng = np.random.default_rng(7 * W + H)
    refs = [_binary(rng, W, H, 4) for _ in range(3)]
    cur = [np.zeros_like(p) for p in refs[0]]
    mbw = W // 16
    for m in range(mbw * (H // 16)):
        mx, my = m % mbw, m // mbw
        src = refs[m % 3]
        for pl, s in ((0, 16), (1, 8), (2, 8)):
            x0, y0, q = mx * s, my * s, s // 2
            for k, (qy, qx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                dx = (k if pl == 0 else 0) if (m & 1) else 0                       # luma quadrants 0..3 pixels to the right of their place
                xs = np.clip(np.arange(x0 + qx * q, x0 + qx * q + q) + dx, 0, src[pl].shape[1] - 1)
                cur[pl][y0 + qy * q:y0 + (qy + 1) * q, x0 + qx * q:x0 + (qx + 1) * q] = src[pl][y0 + qy * q:y0 + (qy + 1) * q][:, xs]
            noise = rng.random((s, s)) < (0.0, 0.02, 0.08, 0.3)[(m // 2) % 4]
            cur[pl][y0:y0 + s, x0:x0 + s] ^= (noise * 255).astype(np.uint8)
    return [refs[0], refs[1], refs[2], tuple(np.ascontiguousarray(p) for p in cur)]


def cases():
    return [("q0", qc.segments((0,) * 4), -1.0), ("q127", qc.segments((127,) * 4), -1.0),
            ("ladder", qc.segments(LADDER, qc.DELTA_SETS["alt"], junk=True), TARGET)]


_oracle = {}


def oracle_results(W, H):
    """{tag: everything the frame leaves} from the oracle alone: computed once, shared by the tests, never changed"""
    if (W, H) not in _oracle:
        frames, out = mixed(W, H), {}
        for target in sorted(set(c[2] for c in cases())):
            ora = Oracle(W, H, target)
            ora.set_segments(cases()[0][1])
            _prepare(ora, frames)
            for tag, sd, t in cases():
                if t == target:
                    out[tag] = _frame(ora, frames, sd, (1, 1))
            ora.close()
        _oracle[(W, H)] = out
    return _oracle[(W, H)]


def differences(W, H):
    frames, bad = mixed(W, H), []
    want = oracle_results(W, H)
    for target in sorted(set(c[2] for c in cases())):
        hip = api.Vp8Hip(W, H, target)
        hip.set_segments(cases()[0][1])
        _prepare(hip, frames)
        for tag, sd, t in cases():
            if t != target:
                continue
            try:
                _compare(_frame(hip, frames, sd, (1, 1)), want[tag], KEYS, f"{W}x{H} {tag}")
            except AssertionError as e:
                bad.append(str(e))
        hip.close()
    return bad


def second_order_differences():
    bad = []
    for name in ("flat_up", "flat_down"):
        frames = [qc.CONTENTS[name][1][0], qc.CONTENTS[name][1][1], qc.CONTENTS[name][1][2], qc.CONTENTS[name][0]]
        sd = qc.segments((0,) * 4)
        res = []
        for be in (api.Vp8Hip(qc.W, qc.H), Oracle(qc.W, qc.H)):
            res.append(_frame(be, frames, sd, (0, 0)))
            be.close()
        dc = res[1]["MB_coeffs"][res[1]["MB_parts"] == 0][:, 24, 0]
        assert dc.size and int(dc.max() if name == "flat_up" else dc.min()) == (2040 if name == "flat_up" else -2040), (name, dc)
        try:
            _compare(res[0], res[1], KEYS, name)
        except AssertionError as e:
            bad.append(str(e))
    return bad


def test_the_contents_hold_what_the_kernels_branch_on():
    """on the oracle's results alone: split and unsplit macroblocks, winners in all three references, the ladder left after one, two and
    four passes under the one target (segment 3 = one pass, 2 = two, 0 = four)"""
    parts, refs, segs = set(), set(), set()
    for W, H in SIZES:
        o = oracle_results(W, H)
        for tag in ("q0", "q127", "ladder"):
            parts |= set(int(v) for v in o[tag]["MB_parts"])
            refs |= set(int(v) for v in o[tag]["MB_reference_frame"])
        segs |= set(int(v) for v in o["ladder"]["MB_segment_id"])
        print(f"{W}x{H}: parts {o['q0']['MB_parts'].tolist()} references {o['q0']['MB_reference_frame'].tolist()} "
              f"ladder segments {o['ladder']['MB_segment_id'].tolist()}")
    assert parts == {0, 1}, parts
    assert len(refs) == 3, refs
    assert {3, 2, 0} <= segs, segs


@pytest.mark.parametrize("W,H", SIZES)
def test_k_mb_p_on_frames_of_one_six_and_nine_macroblocks(W, H):
    bad = differences(W, H)
    assert not bad, bad


def test_k_mb_p_with_the_second_order_dc_at_both_bounds():
    bad = second_order_differences()
    assert not bad, bad
