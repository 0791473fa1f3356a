"""The canvas rule on the host (vp8host_compose_frame; include/vp8hip_host.h, "CANVAS"): the plain C++ form against the numpy
restatement (tests/compose_ref.py) byte for byte on the cases the GPU suite runs, the identities the rule promises, the one validity
rule of the intake settings on the canvas fields -- every refusal, every excluded combination both ways round -- and the stand-alone
program that runs the rule under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import compose_ref as R
from test_scale_cpu import AREA, LANCZOS, lib_taps, ref_scale_frame
from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include")]


def same(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


def random_frame(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_host_form_equals_the_restatement(name, pitched):
    _, (pw, ph), tiles, bg, _ = R.CASES[name]
    frames = R.case_frames(name, pitched=pitched)
    same(api.compose_frame(pw, ph, tiles, frames, bg), R.ref_compose(pw, ph, tiles, frames, bg), name)


@pytest.mark.parametrize("kind", [AREA, LANCZOS])
def test_one_full_picture_tile_is_the_scaler(kind):
    f = random_frame(130, 98, 1)
    same(api.compose_frame(66, 34, [(130, 98, 0, 0, 66, 34, kind)], [f]), ref_scale_frame(*f, 66, 34, kind, lib_taps), "130x98 -> 66x34")


@pytest.mark.parametrize("kind", [AREA, LANCZOS])
def test_a_one_to_one_tile_is_its_input(kind):
    f = random_frame(64, 48, 2)
    same(api.compose_frame(64, 48, [(64, 48, 0, 0, 64, 48, kind)], [f]), f, "1:1")
    # ... and inside a larger picture, over the background
    y, u, v = api.compose_frame(80, 64, [(64, 48, 10, 6, 64, 48, kind)], [f], bg=(1, 2, 3))
    same((y[6:54, 10:74], u[3:27, 5:37], v[3:27, 5:37]), f, "1:1 at (10, 6)")
    assert (y[:6] == 1).all() and (y[54:] == 1).all() and (y[:, :10] == 1).all() and (y[:, 74:] == 1).all()
    assert (u[:3] == 2).all() and (u[:, 37:] == 2).all() and (v[27:] == 3).all() and (v[:, :5] == 3).all()


def test_an_absent_tile_leaves_the_background_and_what_is_under_it():
    f = random_frame(32, 32, 3)
    tiles = [(32, 32, 0, 0, 32, 32, AREA), (32, 32, 16, 16, 16, 16, AREA)]
    none = api.compose_frame(48, 32, tiles, [None, None], bg=(200, 100, 50))
    assert (none[0] == 200).all() and (none[1] == 100).all() and (none[2] == 50).all()
    under = api.compose_frame(48, 32, tiles, [f, None], bg=(200, 100, 50))
    same(under, api.compose_frame(48, 32, tiles[:1], [f], bg=(200, 100, 50)), "the second tile absent")
    same((under[0][:, :32], under[1][:, :16], under[2][:, :16]), f, "the first tile whole")


def test_tile_order_decides_an_overlap():
    a, b = random_frame(32, 32, 4), random_frame(32, 32, 5)
    ta, tb = (32, 32, 0, 0, 32, 32, AREA), (32, 32, 16, 8, 32, 32, AREA)
    ab = api.compose_frame(48, 40, [ta, tb], [a, b])
    ba = api.compose_frame(48, 40, [tb, ta], [b, a])
    assert np.array_equal(ab[0][8:32, 16:32], b[0][:24, :16]) and np.array_equal(ba[0][8:32, 16:32], a[0][8:32, 16:32])
    assert np.array_equal(ab[1][4:16, 8:16], b[1][:12, :8]) and np.array_equal(ba[2][4:16, 8:16], a[2][4:16, 8:16])
    same(ab, R.ref_compose(48, 40, [ta, tb], [a, b]), "a under b")
    same(ba, R.ref_compose(48, 40, [tb, ta], [b, a]), "b under a")
    assert not np.array_equal(ab[0], ba[0])


def test_the_host_form_refuses_what_the_rule_refuses():
    f = random_frame(32, 32, 6)
    ok = (32, 32, 0, 0, 32, 32, AREA)
    api.compose_frame(32, 32, [ok], [f])
    for pw, ph, tile, bg in [(32, 32, (32, 32, 1, 0, 32, 32, AREA), R.BG), (32, 32, (32, 32, 2, 0, 32, 32, AREA), R.BG), (34, 32, (32, 32, 0, 0, 34, 32, AREA), R.BG),
                             (32, 32, ok[:6] + (2,), R.BG), (32, 32, ok, (256, 0, 0)), (32, 32, ok, (0, 0, -1)), (33, 32, ok, R.BG), (0, 0, ok, R.BG)]:
        with pytest.raises(ValueError):
            api.compose_frame(pw, ph, [tile], [f], bg)
    with pytest.raises(ValueError):
        api.compose_frame(64, 64, [(16, 16, 0, 0, 16, 16, AREA)] * 17, [random_frame(16, 16, 7)] * 17)


# ---- the one validity rule on the canvas fields ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("canvas_rule") / "canvas_rule_check")
    subprocess.run(SAN + [os.path.join(ROOT, "scripts", "native", "canvas_rule_check.cpp"), os.path.join(ROOT, "vp8oclenc_amd", "csrc", "vp8_host.cpp"), "-o", exe],
                   check=True, timeout=600)

    def verdicts(cases):
        """cases: dicts of the settings' fields (W, H default 64 x 48; tiles: a list of 7-tuples) -> one list of words per case"""
        lines = []
        for c in cases:
            tiles = c.get("tiles", [])
            head = [c.get(k, d) for k, d in (("W", 64), ("H", 48), ("src_w", 0), ("src_h", 0), ("in_w", 0), ("in_h", 0), ("scale_kind", 0), ("src_fmt", 0), ("win_on", 0),
                                             ("or_turns", 0), ("or_mirror", 0), ("di_mode", 0))] + list(c.get("bg", R.BG)) + [c.get("n_tiles", len(tiles))]
            lines.append(" ".join(str(int(x)) for x in head + [x for t in tiles for x in t]))
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return verdicts


OK_TILE = (128, 96, 0, 0, 64, 48, AREA)


def test_the_rule_accepts_the_cases_and_refuses_bad_tiles(rule):
    good = [dict(W=c[0][0], H=c[0][1], src_w=c[1][0], src_h=c[1][1], tiles=c[2], bg=c[3]) for c in R.CASES.values()]
    good += [dict(tiles=[OK_TILE]), dict(tiles=[(64, 48, 0, 0, 64, 48, LANCZOS)] * 16), dict(tiles=[(16384, 96, 0, 0, 1024, 48, AREA)], W=1024), dict(tiles=[OK_TILE], bg=(0, 255, 0))]
    for c, v in zip(good, rule(good)):
        assert v[0] == "ok" and "plain" not in v, (c, v)
    t = OK_TILE
    bad = [dict(tiles=[(129, 96, 0, 0, 64, 48, AREA)]), dict(tiles=[(128, 97, 0, 0, 64, 48, AREA)]), dict(tiles=[(128, 96, 1, 0, 62, 48, AREA)]),      # odd values
           dict(tiles=[(128, 96, 0, 1, 64, 46, AREA)]), dict(tiles=[(128, 96, 0, 0, 63, 48, AREA)]), dict(tiles=[(128, 96, 0, 0, 64, 47, AREA)]),
           dict(tiles=[(128, 96, 2, 0, 64, 48, AREA)]), dict(tiles=[(128, 96, 0, 2, 64, 48, AREA)]), dict(tiles=[(128, 96, -2, 0, 64, 48, AREA)]),      # outside the picture
           dict(tiles=[(128, 96, 0, -2, 32, 32, AREA)]), dict(tiles=[t], src_w=62, src_h=48), dict(tiles=[t], src_w=64, src_h=46),
           dict(tiles=[(128, 96, 0, 0, 0, 48, AREA)]), dict(tiles=[(128, 96, 0, 0, 64, 0, AREA)]),
           dict(tiles=[(62, 96, 0, 0, 64, 48, AREA)]), dict(tiles=[(128, 46, 0, 0, 64, 48, AREA)]),      # w > in_w, h > in_h: no upscaling
           dict(tiles=[(16386, 96, 0, 0, 1024, 48, AREA)], W=1024), dict(tiles=[(128, 16386, 0, 0, 64, 1024, AREA)], H=1024),
           dict(tiles=[(128, 96, 0, 0, 64, 48, 2)]), dict(tiles=[(128, 96, 0, 0, 64, 48, -1)]),
           dict(tiles=[(66, 48, 0, 0, 2, 48, AREA)]), dict(tiles=[(132, 96, 0, 0, 4, 48, AREA)]),      # pairs vp8host_scale_taps refuses: 33 taps
           dict(tiles=[(384, 288, 0, 0, 64, 48, LANCZOS)]), dict(tiles=[(64, 48, 0, 0, 64, 2, LANCZOS)]),      # Lanczos at 6:1; a chroma plane of one row
           dict(tiles=[(16, 16, 0, 0, 16, 16, AREA)] * 17, n_tiles=17),
           dict(tiles=[t], bg=(256, 128, 128)), dict(tiles=[t], bg=(16, -1, 128)), dict(tiles=[t], bg=(16, 128, 300)),
           dict(tiles=[t, (128, 96, 2, 0, 64, 48, AREA)])]      # a bad tile behind a good one
    for c, v in zip(bad, rule(bad)):
        assert v[0] == "refused", (c, v)


def test_the_rule_excludes_both_ways_round(rule):
    """the scaler's incoming size, a source format, a window, an orientation and the deinterlacer: each valid on its own, each refused
    with a canvas -- the candidate is complete, so which setter came last plays no part -- and a canvas keeps a context out of hidden
    alt-ref frames, by-reference splits and batches"""
    others = [dict(in_w=128, in_h=96), dict(in_w=128, in_h=96, scale_kind=1), dict(src_fmt=1), dict(src_fmt=16), dict(win_on=1), dict(or_turns=2), dict(or_turns=1, W=48, H=48),
              dict(or_mirror=1), dict(di_mode=1), dict(di_mode=2)]
    canvas = dict(tiles=[(64, 48, 0, 0, 48, 48, AREA)])
    alone = rule(others)
    both = rule([dict(o, **canvas) for o in others])
    for o, a, b in zip(others, alone, both):
        assert a[0] == "ok" and "plain" in a and "batch" not in a, (o, a)
        assert b[0] == "refused", (o, b)
    v = rule([canvas, dict(canvas, src_w=60, src_h=48), {}])
    assert v[0] == ["ok", "arf", "shard", "batch"] and v[1] == ["ok", "arf", "shard", "batch"] and v[2] == ["ok", "plain"]
    # the canonical form: no canvas leaves nothing behind
    assert rule([dict(tiles=[OK_TILE], n_tiles=0, bg=(1, 2, 3))])[0] == ["ok", "plain"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_host_rule_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "compose_sanitize")
    subprocess.run(SAN + [os.path.join(ROOT, "scripts", "native", "compose_sanitize.cpp"), os.path.join(ROOT, "vp8oclenc_amd", "csrc", "vp8_host.cpp"), "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("clean"), r.stdout + r.stderr


def test_the_library_exports_the_entry_points():
    lib = api.load_library()
    for name in ("vp8hip_set_canvas", "vp8hip_compose_current_device", "vp8hip_compose_current_host", "vp8host_compose_frame", "vp8drv_set_canvas",
                 "vp8drv_encode_frame_tiles_device", "vp8drv_encode_frame_tiles_host"):
        assert hasattr(lib, name), name
    assert api.MAX_TILES == 16 and api.parse_tile("a:b.yuv:352x288:88:0:88:72:lanczos")[0] == "a:b.yuv"
    t = api.parse_tile("cam.yuv:1280x720:0:0:960:540")[1]
    assert (t.in_w, t.in_h, t.x, t.y, t.w, t.h, t.filter) == (1280, 720, 0, 0, 960, 540, AREA)
    with pytest.raises(ValueError):
        api.parse_tile("cam.yuv:1280x720:0:0:960")
