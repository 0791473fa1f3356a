"""The two macroblock kernels (k_mb_p, k_mb_p_conformant: kernels_mb.hip) against the CPU oracle over the whole
quantiser space, on content that takes their narrow arithmetic to the bounds its comments state (tests/quantiser_cases.py; what the cases
reach is asserted on the CPU in test_quantiser_space_cpu.py): tdiv's reciprocal multiply with numerators up to 16320 and every quantiser
the tables and the index deltas can produce, the transform's rotations on packed 16-bit halves with residuals of +-255 everywhere, the
24-bit multiplies of the dequantiser and the inverse transform, the second-order transform spread over sixteen lanes, the SSIM gate and
the four-pass segment loop leaving at every pass.

One context per content (and SSIM target): between cases only the segment data changes, and LAST is uploaded again because the loop
filter overwrote it.  Everything the frame leaves is compared bit for bit, MB_SSIM by its bit pattern.  The conformant kernel differs
only in the predictor: it runs on the inverse contents, where the last three filtered lines leave 0..255.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

import quantiser_cases as qc
from oracle_lib import Oracle
from test_gpu_parity import _compare
from test_gpu_search_saturating import _prepare
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu

KEYS = ["MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs", "MB_segment_id", "MB_SSIM", "prefilter_Y", "prefilter_U", "prefilter_V",
        "MB_non_zero_coeffs", "mb_mask", "recon_Y", "recon_U", "recon_V"]


def _frames(name):
    cur, refs, flags = qc.CONTENTS[name]
    return [refs[0], refs[1], refs[2], cur], flags      # the order _prepare takes: LAST, GOLDEN, ALTREF sources, current


def _frame(be, frames, sd, flags):
    """one inter frame and its loop filter on a prepared context: everything the frame leaves"""
    be.set_segments(sd)
    be.upload_last(*frames[0])
    be.upload_current(*frames[3])
    be.inter_transform(0, 0, *flags)
    res = be.download_results(recon=True)
    be.prepare_filter_mask(want_nz=False)
    be.loop_filter()
    if isinstance(be, Oracle):
        res.update(be.filter_outputs())
    else:
        res["mb_mask"] = be.debug(api.DBG_MB_MASK)
        res["MB_non_zero_coeffs"] = be.debug(api.DBG_MB_NZ)
        res["recon_Y"], res["recon_U"], res["recon_V"] = be.download_last()
    return res


def differences(name, cases, conformant=False):
    """[message] of the cases in which the HIP path and the oracle differ on content `name`"""
    frames, flags = _frames(name)
    H, W = frames[3][0].shape
    bad = []
    Oracle.lib().vp8o_set_conformant_stream(int(conformant))
    try:
        for target in sorted(set(c[2] for c in cases)):
            hip, ora = api.Vp8Hip(W, H, target), Oracle(W, H, target)
            if conformant:
                hip.conformant_stream(True)
            for be in (hip, ora):
                be.set_segments(cases[0][1])
                if flags != (0, 0):
                    _prepare(be, frames)
            for tag, sd, t in cases:
                if t != target:
                    continue
                h, o = _frame(hip, frames, sd, flags), _frame(ora, frames, sd, flags)
                try:
                    _compare(h, o, KEYS, f"{name} {tag}{' conformant' if conformant else ''}")
                except AssertionError as e:
                    bad.append(str(e))
            hip.close()
            ora.close()
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)
    return bad


@pytest.mark.parametrize("name", list(qc.CONTENTS))
def test_every_index(name):
    bad = differences(name, qc.index_sweep())
    assert not bad, f"{len(bad)} of 128 indices differ: {bad[:3]}"


@pytest.mark.parametrize("name", list(qc.CONTENTS))
def test_index_deltas_at_both_ends_of_the_clamp(name):
    cases = qc.delta_sets()
    bad = differences(name, cases)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ: {bad[:3]}"


@pytest.mark.parametrize("name", qc.LOOP_CONTENTS + ["squares_inv_3refs", "one_mb"])
def test_ladders_and_targets(name):
    cases = qc.ladders()
    bad = differences(name, cases)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ: {bad[:3]}"


@pytest.mark.parametrize("name", qc.INVERSE_CONTENTS)
def test_conformant_predictor(name):
    cases = qc.index_sweep(8) + qc.delta_sets() + qc.ladders()
    bad = differences(name, cases, conformant=True)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ: {bad[:3]}"


# ---- a batched launch: segment data is a per-member pointer ------------------------------------------------------------------------
def test_a_batch_whose_members_differ_in_content_and_segment_data():
    target = 0.90
    members = [("squares_inv_3refs", qc.ladders((target,))[0][1]), ("pixels_inv", qc.ladders((target,))[1][1]),
               ("hadamard", qc.segments((0,) * 4, qc.DELTA_SETS["minus"], junk=True)),
               ("flat_down", qc.segments((127,) * 4, qc.DELTA_SETS["plus"], junk=True))]
    n = len(members)
    want = []
    for name, sd in members:
        frames, flags = _frames(name)
        o = Oracle(qc.W, qc.H, target)
        o.set_segments(sd)
        _prepare(o, frames)
        o.inter_transform(0, 0, *flags)
        want.append(o.download_results(recon=True))
        o.close()
    assert len(set(w["MB_coeffs"].tobytes() for w in want)) == n
    lib = api.load_library()
    ctxs = [api.Vp8Hip(qc.W, qc.H, target) for _ in range(n)]
    hb = C.c_void_p()
    try:
        for m, (name, sd) in zip(ctxs, members):
            m.set_segments(sd)
            _prepare(m, _frames(name)[0])
        lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
        lib.vp8hip_batch_inter_transform.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 5
        lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
        lib.vp8hip_batch_destroy.restype = None
        assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * n)(*[m.h for m in ctxs]), n) == 0
        ints = lambda v: (C.c_int * n)(*v)
        flags = [_frames(name)[1] for name, _ in members]
        assert lib.vp8hip_batch_inter_transform(hb, None, ints([0] * n), ints([0] * n), ints([f[0] for f in flags]), ints([f[1] for f in flags])) == 0
        api.device_synchronize()
        for i, m in enumerate(ctxs):
            _compare(m.download_results(recon=True), want[i], KEYS[:9], f"member {i} ({members[i][0]})")
    finally:
        if hb:
            lib.vp8hip_batch_destroy(hb)
        for m in ctxs:
            m.close()


# ---- the entropy stage on the same frames: coefficients larger than any inter frame of test_gpu_entropy.py -----------------------------
@pytest.mark.parametrize("name,q", [("flat_up", 0), ("hadamard", 0), ("squares_inv", 0), ("squares_inv", 127)])
def test_entropy_stage_on_these_frames(name, q):
    from entropy_cases import nz_counts, run_stage
    from test_gpu_entropy import check_counts
    frames, flags = _frames(name)
    sd = qc.segments((q,) * 4)
    ora = Oracle(qc.W, qc.H)
    ora.set_segments(sd)
    ora.upload_last(*frames[0])
    ora.upload_current(*frames[3])
    ora.inter_transform(0, 0, *flags)
    r = ora.download_results(recon=False)
    ora.close()
    coeffs, parts = np.ascontiguousarray(r["MB_coeffs"]), np.ascontiguousarray(r["MB_parts"])
    big = int(np.abs(coeffs[:, 24][parts == 0].astype(np.int32)).max()) if (parts == 0).any() else 0
    if name in ("flat_up", "hadamard"):
        assert big >= 1091, big          # DCT_CAT6 with its top extra bit set
    nz = nz_counts(coeffs, parts)
    hip = api.Vp8Hip(qc.W, qc.H)
    hip.set_segments(sd)
    hip.upload_last(*frames[0])
    hip.upload_current(*frames[3])
    hip.inter_transform(0, 0, *flags)
    assert np.array_equal(hip.download_results(recon=False)["MB_coeffs"], coeffs)
    assert np.array_equal(hip.debug(api.DBG_MB_NZ), nz)
    for P in (1, 2, 8):
        exp = run_stage(Oracle.stages(), coeffs, parts, nz, qc.W // 16, qc.H // 16, P)
        check_counts(hip, exp, nz, P, f"{name} q{q} P{P}", parts=parts)
    hip.close()

