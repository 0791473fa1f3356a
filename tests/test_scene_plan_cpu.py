"""vp8host_scene_plan (include/vp8hip_host.h): the serial loop's key-frame schedule with scene detection on, from the chroma differences
of a file's frames and the GOP length.  Against a Python restatement of the rule, against the frame loop's own functions stepped one by
one through their bindings, on a constructed case whose result follows from the rule, and under the host sanitizers; and
gop_shard.chunks_from_keys, which cuts the chunks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from vp8oclenc_amd import api, gop_shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_ref(ud, vd, g):
    """the rule in Python, nothing shared with the library: scene_change() (vp8enc.cpp:285-310) and the key-frame counter (:364-374,
    intra_part.h:1091-1098)"""
    until_key, holdover, last_key_detect = 1, False, 0
    key, scene = [], []
    for t in range(len(ud)):
        until_key -= 1
        k, s = until_key < 1, False
        if not k:      # only a frame that would be an inter frame is looked at
            detect = ud[t] > 7 or vd[t] > 7 or ud[t] + vd[t] > 10
            recent = t - last_key_detect < 4
            if detect and recent:
                last_key_detect, holdover = t, True
            elif detect:
                k = s = True
            elif holdover and not recent:
                holdover, k, s = False, True, True
        if k:
            last_key_detect, until_key = t, g
        key.append(k)
        scene.append(s)
    return np.array(key, bool), np.array(scene, bool)


def plan_stepped(ud, vd, g):
    """the driver's loop through the bindings of the functions it calls"""
    gop, st = api.Gop(g, 5), api.SceneState()
    key, scene = [], []
    for t in range(len(ud)):
        s_ = gop.next()
        k, s = bool(s_.current_is_key), False
        if not k and api.scene_change(st, int(ud[t]), int(vd[t]), s_.frame_number):
            k = s = True
        if k:
            st.last_key_detect = gop.s.frame_number
            gop.key_coded()
        gop.frame_done()
        key.append(k)
        scene.append(s)
    return np.array(key, bool), np.array(scene, bool)


def random_differences(rng, n, p=0.15):
    cut = rng.random(n) < p
    kind = rng.integers(0, 3, n)
    ud = np.where(cut & (kind == 0), rng.integers(8, 256, n), rng.integers(0, 6, n))
    vd = np.where(cut & (kind == 1), rng.integers(8, 256, n), rng.integers(0, 5, n))
    both = cut & (kind == 2)      # neither above 7, the sum above 10
    ud, vd = np.where(both, 6, ud), np.where(both, 5 + rng.integers(0, 3, n), vd)
    return ud.astype(np.int32), vd.astype(np.int32)


def test_against_the_python_restatement():
    rng = np.random.default_rng(3)
    for _ in range(3000):
        n, g = int(rng.integers(0, 80)), int(rng.integers(1, 20))
        ud, vd = random_differences(rng, n)
        key, scene = api.scene_plan(ud, vd, g)
        rk, rs = plan_ref(ud, vd, g)
        assert np.array_equal(key, rk) and np.array_equal(scene, rs), (g, ud, vd)


def test_against_the_loops_own_functions_stepped_one_by_one():
    rng = np.random.default_rng(4)
    cuts = 0
    for i in range(3000):
        g = 1 + i % 12
        ud, vd = random_differences(rng, 60)
        key, scene = api.scene_plan(ud, vd, g)
        sk, ss = plan_stepped(ud, vd, g)
        assert np.array_equal(key, sk) and np.array_equal(scene, ss), (g, ud, vd)
        assert key[0] and not scene[0] and not (scene & ~key).any()
        cuts += int(scene.sum())
    assert cuts > 3000      # the sequences do have cuts


CONSTRUCTED_CUTS, CONSTRUCTED_KEYS = (6, 8, 21, 22, 33), [0, 6, 12, 21, 26, 33]


def test_the_constructed_case():
    """g = 9, 34 frames, cuts at 6, 8, 21, 22 and 33.  By the rule: 0 is scheduled; 6 is detected, more than three frames after 0; 8 is
    detected within four frames of 6, so it is held over (and moves last_key_detect to 8); the hold-over comes due at the first frame
    four or more after 8 that is looked at: 12, a frame without any difference; 21 = 12 + 9 is a scheduled key frame, so the cut on it is
    never looked at; 22 is detected within four frames of 21: held over, due at 26; 30 would be scheduled only at 35; 33 is detected,
    seven frames after 26.  The last chunk has one frame."""
    ud, vd = np.zeros(34, np.int32), np.zeros(34, np.int32)
    ud[list(CONSTRUCTED_CUTS)] = 40
    key, scene = api.scene_plan(ud, vd, 9)
    sk, _ = plan_stepped(ud, vd, 9)
    assert np.array_equal(key, sk)
    assert list(np.flatnonzero(key)) == CONSTRUCTED_KEYS
    assert list(np.flatnonzero(scene)) == [6, 12, 26, 33]      # (0 and 21 are the schedule's)
    assert gop_shard.chunks_from_keys(key) == [(0, 6), (6, 6), (12, 9), (21, 5), (26, 7), (33, 1)]
    ud[21] = 0      # the cut on the scheduled key frame was never looked at: without it, the same plan
    assert np.array_equal(api.scene_plan(ud, vd, 9)[0], key)


def test_without_cuts_the_plan_is_the_fixed_one():
    for n, g in ((0, 5), (1, 1), (23, 5), (36, 12), (7, 30)):
        key, scene = api.scene_plan(np.zeros(n, np.int32), np.zeros(n, np.int32), g)
        assert not scene.any() and gop_shard.chunks_from_keys(key) == gop_shard.gop_chunks(n, g)


def test_refusals_and_symbols():
    with pytest.raises(ValueError):
        api.scene_plan(np.zeros(4, np.int32), np.zeros(4, np.int32), 0)
    with pytest.raises(ValueError):
        api.scene_plan(np.zeros(4, np.int32), np.zeros(5, np.int32), 3)
    with pytest.raises(ValueError):
        gop_shard.chunks_from_keys([0, 1, 0])
    assert gop_shard.chunks_from_keys([]) == []
    lib = api.load_library()
    for name in ("vp8host_scene_plan", "vp8hip_batch_chroma_change_async", "vp8drv_batch_scan_frame_device", "vp8drv_batch_scan_frame_host", "vp8drv_batch_scan_result"):
        assert name in api.ABI_SYMBOLS and hasattr(lib, name), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_host_rule_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "scene_plan_sanitize")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "native", "scene_plan_sanitize.cpp"), os.path.join(ROOT, "vp8oclenc_amd", "csrc", "vp8_host.cpp"),
                    "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("clean"), r.stdout + r.stderr
