"""The temporal denoiser's contract without a GPU: the numpy restatement of include/vp8hip_host.h's rule (tests/denoise_ref.py) against
vp8host_denoise_frame byte for byte, inputs that make every branch occur (asserted on the restatement itself), the invariants the
rule promises, and the ABI: new entry points, vp8drv_config and the ABI version unchanged.  tests/test_gpu_denoise.py holds the
kernel to the same restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as ref
from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(16, 16), (48, 32), (64, 48)]
LEVELS = [1, 2, 3]
NEW_SYMBOLS = ["vp8hip_set_denoise", "vp8hip_denoise_restart", "vp8hip_denoise_result", "vp8host_denoise_frame", "vp8drv_set_denoise",
               "vp8drv_get_denoise_stats"]


def _run_host(frames, level, restart_at=()):
    """the sequence through vp8host_denoise_frame -> list of (out, filtered)"""
    hist = [np.zeros_like(p) for p in frames[0]]
    have, res = False, []
    for t, f in enumerate(frames):
        if t in restart_at:
            have = False
        out, n = api.denoise_frame(f, hist, level, have)
        have = True
        for a, b in zip(hist, out):
            assert np.array_equal(a, b)      # the whole output frame is the new history
        res.append((out, n))
    return res


def _run_ref(frames, level, restart_at=()):
    d, res = ref.Denoiser(level), []
    for t, f in enumerate(frames):
        if t in restart_at:
            d.restart()
        res.append(d.take(f))
    return res


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_host_function_equals_the_restatement_byte_for_byte(w, h, level):
    for name, frames in ref.sequences(w, h, seed=w + level).items():
        assert len(frames) == 5
        got, want = _run_host(frames, level), _run_ref(frames, level)
        for t, ((go, gn), (wo, wn, _)) in enumerate(zip(got, want)):
            for p in range(3):
                assert np.array_equal(go[p], wo[p]), (name, t, p)
            assert gn == wn, (name, t)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_the_inputs_reach_every_branch(w, h, level):
    seqs = ref.sequences(w, h, seed=w + level)
    total = (w // 16) * (h // 16)
    # static picture + noise <= 3: every block filtered, the output is the history
    res = _run_ref(seqs["static_noise"], level)
    for t in range(1, 5):
        out, n, info = res[t]
        assert n == total and info["filtered_u"].all() and info["filtered_v"].all()
        for p in range(3):
            assert np.array_equal(out[p], res[t - 1][0][p])
    # the stripe that moves 8 samples: a macroblock copied through the SAD bound alone
    hits = 0
    for out, n, info in _run_ref(seqs["moving_stripe"], level)[1:]:
        by_sad = (np.abs(info["T"]) <= ref.SUM_Y) & (info["sad"] > ref.SAD_Y)
        assert not (info["filtered"] & by_sad).any()
        hits += int(by_sad.sum())
    assert hits > 0
    # +5 everywhere: copied through the sum bound alone (256 * 3 > 512 at level 1)
    frames = seqs["brightness_step"]
    for t, (out, n, info) in enumerate(_run_ref(frames, level)[1:], 1):
        assert n == 0 and (info["sad"] == 1280).all() and (np.abs(info["T"]) >= 768).all()
        assert np.array_equal(out[0], frames[t][0])
    # luma filtered, U copied, V filtered
    frames = seqs["chroma_step"]
    for t, (out, n, info) in enumerate(_run_ref(frames, level)[1:], 1):
        assert n == total and not info["filtered_u"].any() and info["filtered_v"].all()
        assert np.array_equal(out[1], frames[t][1])
    # some and not all
    if total > 1:
        assert any(0 < n < total for _, n, _ in _run_ref(seqs["mixed"], level))
    # every branch of the per-sample step in one sequence
    seen = set()
    d = ref.Denoiser(level)
    prev = None
    for f in seqs["wild"]:
        if prev is not None:
            a = np.abs(prev[0].astype(int) - f[0].astype(int))
            seen |= {0 if x <= 2 + level else (1 if x <= 7 else (2 if x <= 15 else 3)) for x in np.unique(a)}
        prev = d.take(f)[0]
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("level", LEVELS)
def test_output_lies_between_source_and_history(level):
    for w, h in GEOMETRIES:
        for name, frames in ref.sequences(w, h, seed=7).items():
            hist = None
            for f in frames:
                fh = [p.copy() for p in (hist or f)]
                out, _ = api.denoise_frame(f, fh, level, hist is not None)
                if hist is not None:
                    for p in range(3):
                        lo, hi = np.minimum(f[p], hist[p]), np.maximum(f[p], hist[p])
                        assert ((out[p] >= lo) & (out[p] <= hi)).all(), (name, p)
                hist = out


def test_level_zero_first_frame_and_restart_are_identities():
    w, h = 48, 32
    frames = ref.sequences(w, h, seed=3)["wild"]
    for f in frames:      # level 0: out = src, nothing filtered, the history untouched (or absent)
        hist = [np.full_like(p, 9) for p in f]
        out, n = api.denoise_frame(f, hist, 0, True)
        assert n == 0 and all(np.array_equal(a, b) for a, b in zip(out, f)) and all((p == 9).all() for p in hist)
        out, n = api.denoise_frame(f, None, 0, False)
        assert n == 0 and all(np.array_equal(a, b) for a, b in zip(out, f))
    for level in LEVELS:
        res = _run_host(frames, level, restart_at=(3,))
        want = _run_ref(frames, level, restart_at=(3,))
        for t in (0, 3):      # the first frame and the one behind a restart pass through and become the history
            assert res[t][1] == 0 and all(np.array_equal(a, b) for a, b in zip(res[t][0], frames[t]))
        assert any(not np.array_equal(res[t][0][0], frames[t][0]) for t in (1, 2, 4))      # (the others do not)
        for (go, gn), (wo, wn, _) in zip(res, want):
            assert gn == wn and all(np.array_equal(a, b) for a, b in zip(go, wo))


def test_bad_arguments_are_refused():
    f = ref.sequences(16, 16)["wild"][0]
    hist = [p.copy() for p in f]
    for level in (-1, 4):
        with pytest.raises(ValueError):
            api.denoise_frame(f, hist, level, True)
    with pytest.raises(ValueError):
        api.denoise_frame(f, None, 1, False)                      # a level without history planes
    with pytest.raises(ValueError):
        api.denoise_frame([p[:8] for p in f], [p[:8].copy() for p in f], 1, True)      # not whole macroblocks


def test_abi_new_entry_points_and_nothing_else_moved():
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.ABI_SYMBOLS, name
    assert C.sizeof(api.DrvConfig) == 88 and api.DrvConfig._fields_[-1][0] == "quality_stats"
    assert C.sizeof(api.DenoiseStats) == 12
    lib.vp8hip_abi_version.restype = C.c_int
    assert lib.vp8hip_abi_version() == 4010 == api.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "vp8hip.h")).read() + open(os.path.join(ROOT, "include", "vp8hip_driver.h")).read() + \
        open(os.path.join(ROOT, "include", "vp8hip_host.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    consts = dict(re.findall(r"#define\s+(VP8HOST_DENOISE_\w+)\s+(\d+)", hdr))
    assert consts == {"VP8HOST_DENOISE_SUM_Y": str(ref.SUM_Y), "VP8HOST_DENOISE_SAD_Y": str(ref.SAD_Y), "VP8HOST_DENOISE_SUM_C": str(ref.SUM_C)}
    assert (api.DENOISE_SUM_Y, api.DENOISE_SAD_Y, api.DENOISE_SUM_C) == (ref.SUM_Y, ref.SAD_Y, ref.SUM_C)
