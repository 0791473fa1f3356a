"""vp8host_aq_segment_map, the variance-adaptive segment map in plain C++ (include/vp8hip_host.h has the rule), against its numpy
restatement tests/aq_ref.py; and the stand-alone program that runs it under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from aq_ref import AQ_W, aq_map, mb_e, noise_blocks, segments_of
from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(y, strength, width=None):
    m, e = api.aq_segment_map(y, strength, width)
    rm, re_, _ = aq_map(y, strength, width)
    assert np.array_equal(e, re_), (e, re_)
    assert np.array_equal(m, rm), (m, rm)
    return m, e


@pytest.mark.parametrize("strength", [1, 2, 3])
@pytest.mark.parametrize("size", [(16, 16), (48, 32), (80, 48)])
def test_random_frames(size, strength):
    w, h = size
    rng = np.random.default_rng(w * 7 + strength)
    check(rng.integers(0, 256, (h, w), dtype=np.uint8), strength)
    check(noise_blocks(w, h, (1, 4, 16, 64), seed=strength), strength)


@pytest.mark.parametrize("strength", [1, 2, 3])
def test_a_flat_frame_is_segment_2(strength):
    m, e = check(np.full((48, 80), 93, np.uint8), strength)
    assert not e.any() and (m == 2).all()


def test_half_black_half_white_is_the_largest_e():
    y = np.zeros((16, 16), np.uint8)
    y[:, 8:] = 255
    m, e = check(y, 2)
    assert e[0] == 239 and m[0] == 2      # (alone in its frame it is the mean)
    y = np.zeros((16, 32), np.uint8)
    y[:8, 16:] = 255
    m, e = check(y, 3)
    assert list(e) == [0, 239] and list(m) == [0, 3]


@pytest.mark.parametrize("strength", [1, 2, 3])
def test_division_rounds_towards_minus_infinity(strength):
    """a frame with a macroblock whose e - E is negative and no multiple of W: truncation would give the segment above"""
    W = AQ_W[strength]
    y = noise_blocks(80, 48, (2, 2, 2, 3, 40), seed=5)
    e = mb_e(y)
    E = int(e.sum()) // e.size
    d = e - E
    odd = (d < 0) & (d % W != 0) & (d > -2 * W)
    assert odd.any(), (E, e)
    trunc = np.clip(2 + np.trunc(d / W).astype(np.int64), 0, 3)
    seg, _ = segments_of(e, strength)
    assert (trunc[odd] != seg[odd]).any()      # the case tells the two roundings apart
    check(y, strength)


@pytest.mark.parametrize("strength", [1, 2, 3])
def test_a_stride_larger_than_the_width(strength):
    rng = np.random.default_rng(11)
    y = rng.integers(0, 256, (32, 48 + 19), dtype=np.uint8)
    m, e = check(y, strength, width=48)
    m2, e2 = api.aq_segment_map(np.ascontiguousarray(y[:, :48]), strength)
    assert np.array_equal(m, m2) and np.array_equal(e, e2)


def test_refusals_and_symbols():
    y = np.zeros((16, 16), np.uint8)
    for s in (0, 4):
        with pytest.raises(ValueError):
            api.aq_segment_map(y, s)
    with pytest.raises(ValueError):
        api.aq_segment_map(np.zeros((24, 16), np.uint8), 1)
    with pytest.raises(ValueError):
        api.aq_segment_map(np.zeros((16, 16), np.uint8), 1, width=32)
    lib = api.load_library()
    for name in ("vp8hip_set_segment_mode", "vp8hip_segment_mode", "vp8hip_set_segment_map_device", "vp8hip_upload_segment_map", "vp8hip_download_segment_map",
                 "vp8host_aq_segment_map", "vp8drv_set_segment_mode", "vp8drv_set_segment_map"):
        assert name in api.ABI_SYMBOLS and hasattr(lib, name), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_host_rule_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "aq_sanitize")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "native", "aq_sanitize.cpp"), os.path.join(ROOT, "vp8oclenc_amd", "csrc", "vp8_host.cpp"),
                    "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("clean"), r.stdout + r.stderr
