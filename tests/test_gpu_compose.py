"""Frames composed of scaled video tiles on the device (vp8hip_set_canvas, vp8hip_compose_current_*, k_compose_b), through the C ABI:
the surfaces against the numpy restatement of tests/compose_ref.py byte for byte -- from device and from host memory, tight and
pitched, at the smallest layouts at which the kernel can still go wrong --, the equivalences with code already trusted (a driver fed
tiles is a plain driver fed vp8host_compose_frame's pictures; one full-picture tile is the scaler; a 1:1 tile is a plain upload), every
refusal with its status code and nothing changed behind it, and the tool."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import compose_ref as R
from test_gpu_scale import assert_surfaces, current_surfaces, expected_surfaces, random_frame, synth_frames
from test_scale_cpu import AREA, LANCZOS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -4


def place(frames, pitched, device):
    """the frames' planes in host or device memory, tight, or pitched (luma rows in_w + 12, chroma rows in_w / 2 + 5 bytes apart) with
    every base 1 byte off a dword -> (tile_planes_array's address form, what keeps the memory alive)"""
    from vp8oclenc_amd import api
    out, keep = [], []
    for f in frames:
        if f is None:
            out.append(None)
            continue
        ptrs, pitches = [], []
        for p, plane in enumerate(f):
            h, w = plane.shape
            pitch = w + ((12 if p == 0 else 5) if pitched else 0)
            nb = pitch * (h - 1) + w
            raw = np.zeros(nb + 8, np.uint8)
            off = ((1 - raw.ctypes.data) % 4 if not device else 1) if pitched else 0      # (device allocations start on 256 bytes)
            np.lib.stride_tricks.as_strided(raw[off:], (h, w), (pitch, 1))[:] = plane
            if device:
                d = api.to_device(raw)
                keep.append(d)
                ptrs.append(d.data_ptr() + off)
            else:
                keep.append(raw)
                ptrs.append(raw.ctypes.data + off)
            assert not pitched or ptrs[-1] % 4 == 1
            pitches.append(pitch if pitched else 0)
        out.append((ptrs[0], ptrs[1], ptrs[2], tuple(pitches)))
    return out, keep


def context(name):
    from vp8oclenc_amd import api
    coded, (pw, ph), tiles, bg, _ = R.CASES[name]
    hip = api.Vp8Hip(*coded)
    if (pw, ph) != coded:
        hip.set_source_size(pw, ph)
    hip.set_canvas(tiles, bg)
    return hip


# ---- 1. the kernel against the restatement, byte for byte ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected():
    """the restatement's surfaces of every case, for the tight and the pitched frames (the same samples): computed once"""
    want = {}
    for name, (coded, (pw, ph), tiles, bg, _) in R.CASES.items():
        want[name] = R.ref_surfaces(coded, pw, ph, tiles, R.case_frames(name), bg)
    return want


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_surfaces_equal_the_restatement(name, expected):
    hip = context(name)
    frames = R.case_frames(name)
    for device in (True, False):
        for pitched in (False, True):
            src, keep = place(frames, pitched, device)
            hip.compose_current(src, device=device)
            hip.synchronize()
            assert_surfaces(current_surfaces(hip), expected[name], f"{name}: {'device' if device else 'host'}, {'pitched' if pitched else 'tight'}")
            del keep
    hip.close()


# ---- 2. equivalences with code already trusted --------------------------------------------------------------------------------------------
def tile_sequences(tiles, n, seed):
    """n frames for every tile: a moving synthetic sequence each, with another scene from frame 4 on"""
    seqs = []
    for k, (in_w, in_h, *_rest) in enumerate(tiles):
        a, b = synth_frames(in_w, in_h, n, seed + 10 * k), synth_frames(in_w, in_h, n, seed + 10 * k + 5)
        seqs.append([(a if t < 4 else b)[t] for t in range(n)])
    return seqs


@pytest.mark.parametrize("name", ["letterbox_ab", "grid_lanczos"])
def test_a_driver_fed_tiles_equals_a_plain_driver_fed_the_composed_pictures(name):
    from vp8oclenc_amd import api
    coded, (pw, ph), tiles, bg, _ = R.CASES[name]
    n = 6
    seqs = tile_sequences(tiles, n, seed=61)
    cfg = dict(gop_size=3, num_partitions=2, scene_detect=1, quality_stats=1)
    size = dict(src_width=pw, src_height=ph) if (pw, ph) != coded else {}
    a, b = api.NativeDriver(*coded, **size, **cfg), api.NativeDriver(*coded, **size, **cfg)
    rng = np.random.default_rng(9)
    layer = rng.integers(0, 256, (12, 20, 4), dtype=np.uint8)
    for d in (a, b):
        d.set_overlay(0, layer, 30, 8, 200)
        d.set_denoise(1)
    a.set_canvas(tiles, bg)
    keys = 0
    for t in range(n):
        frames = [None if (name == "letterbox_ab" and t == 2 and k == 1) else s[t] for k, s in enumerate(seqs)]      # once a participant without video
        a.encode_tiles(frames, device=False) if t & 1 else encode_tiles_device(a, frames)
        b.encode_frame_host(*api.compose_frame(pw, ph, tiles, frames, bg))
        fa, fb = a.get_frame(), b.get_frame()
        assert fa == fb, f"frame {t}: {len(fa)} vs {len(fb)} bytes"
        keys += not (fa[0] & 1)
        for p, q in zip(a.hip.download_last(), b.hip.download_last()):
            assert np.array_equal(p, q), t
        assert bytes(a.frame_quality()) == bytes(b.frame_quality()), t
    assert keys >= 2
    assert bytes(a.quality_summary()) == bytes(b.quality_summary())
    sa, sb = a.stats(), b.stats()
    assert (sa.key_frames, sa.inter_frames, sa.scene_changes) == (sb.key_frames, sb.inter_frames, sb.scene_changes)
    a.close()
    b.close()


def encode_tiles_device(drv, frames):
    src, keep = place(frames, False, True)
    key = drv.encode_tiles(src, device=True)
    drv.hip.synchronize()      # (the planes are read on the context's stream: they stay until it has got there)
    del keep
    return key


@pytest.mark.parametrize("kind", [AREA, LANCZOS])
def test_one_full_picture_tile_gives_the_scalers_surfaces(kind):
    from vp8oclenc_amd import api
    src, dst, coded = (130, 98), (66, 34), (80, 48)
    f = random_frame(*src, 71)
    s = api.Vp8Hip(*coded)
    s.set_source_scaling(src[0], src[1], dst[0], dst[1], kind)
    s.upload_current(*f)
    want = current_surfaces(s)
    s.close()
    assert_surfaces(want, expected_surfaces(f, dst, kind), "the scaler itself")
    c = api.Vp8Hip(*coded)
    c.set_source_size(*dst)
    c.set_canvas([(src[0], src[1], 0, 0, dst[0], dst[1], kind)])
    c.compose_current([f])
    assert_surfaces(current_surfaces(c), want, "one full-picture tile")
    c.close()


def test_a_one_to_one_tile_gives_a_plain_uploads_surfaces():
    from vp8oclenc_amd import api
    for coded, pic in (((64, 48), (64, 48)), ((80, 48), (78, 46))):
        f = random_frame(*pic, 72)
        p = api.Vp8Hip(*coded)
        if pic != coded:
            p.set_source_size(*pic)
        p.upload_current(*f)
        want = current_surfaces(p)
        p.close()
        for kind in (AREA, LANCZOS):
            c = api.Vp8Hip(*coded)
            if pic != coded:
                c.set_source_size(*pic)
            c.set_canvas([(pic[0], pic[1], 0, 0, pic[0], pic[1], kind)])
            c.compose_current([f])
            assert_surfaces(current_surfaces(c), want, f"1:1 {pic} in {coded}, filter {kind}")
            c.close()


@pytest.mark.parametrize("kind", [AREA, LANCZOS])
def test_a_one_to_one_tile_off_every_unit_equals_the_restatement(kind):
    """equal sizes are copied, not scaled (the area filter) or scaled by seven taps that are the identity (Lanczos-3): at (10, 6) the
    rectangle starts off a dword in luma and chroma, crosses output-tile seams and ends two samples behind a dword"""
    from vp8oclenc_amd import api
    tiles, bg, f = [(62, 48, 10, 6, 62, 48, kind), (32, 32, 44, 30, 32, 32, kind)], (1, 2, 3), [random_frame(62, 48, 76), random_frame(32, 32, 77)]
    want = R.ref_surfaces((80, 64), 78, 62, tiles, f, bg)
    c = api.Vp8Hip(80, 64)
    c.set_source_size(78, 62)
    c.set_canvas(tiles, bg)
    for device in (True, False):
        for pitched in (False, True):
            src, keep = place(f, pitched, device)
            c.compose_current(src, device=device)
            c.synchronize()
            assert_surfaces(current_surfaces(c), want, f"1:1 at (10, 6), filter {kind}, {'device' if device else 'host'}, {'pitched' if pitched else 'tight'}")
            del keep
    c.close()


def test_changing_the_layout_between_frames_gives_what_fresh_contexts_give(expected):
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(64, 48)
    plain = random_frame(64, 48, 73)
    for name in ("identity_lanczos", "chunking", "identity_area"):      # (all coded 64 x 48)
        _, _, tiles, bg, _ = R.CASES[name]
        hip.set_canvas(tiles, bg)
        hip.compose_current(R.case_frames(name))
        assert_surfaces(current_surfaces(hip), expected[name], name)
        if name == "chunking":      # ... and out of the canvas and back into it
            hip.set_canvas([])
            hip.upload_current(*plain)
            assert_surfaces(current_surfaces(hip), plain, "no canvas")
    hip.close()


# ---- 3. refusals: the status code, and nothing has changed -----------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(expected):
    from vp8oclenc_amd import api
    name = "grid_area"
    coded, _, tiles, bg, _ = R.CASES[name]
    frames = R.case_frames(name)
    hip = context(name)
    lib = hip.lib
    vp = C.c_void_p
    lib.vp8hip_set_canvas.argtypes = [vp, vp] + [C.c_int] * 4
    lib.vp8hip_canvas_tiles.argtypes = [vp]
    for fn, n in (("vp8hip_set_source_scaling", 5), ("vp8hip_set_source_format", 1), ("vp8hip_set_source_orientation", 2), ("vp8hip_set_deinterlace", 2)):
        getattr(lib, fn).argtypes = [vp] + [C.c_int] * n
    lib.vp8hip_set_source_window.argtypes = [vp, vp, C.c_int, C.c_int]
    for fn in ("vp8hip_set_current_device", "vp8hip_upload_current", "vp8hip_prefetch_current"):
        getattr(lib, fn).argtypes = [vp] * 4
    lib.vp8hip_arf_filter_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    lib.vp8hip_shard_init.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.vp8hip_batch_create.argtypes = [vp, vp, C.c_int]
    lib.vp8hip_compose_current_host.argtypes = [vp, vp]
    lib.vp8hip_compose_current_device.argtypes = [vp, vp]

    def unchanged(what):
        assert lib.vp8hip_canvas_tiles(hip.h) == 4, what
        hip.compose_current(frames)
        assert_surfaces(current_surfaces(hip), expected[name], what)

    # an invalid candidate
    for bad in ([(352, 288, 1, 0, 88, 72, AREA)], [(352, 288, 90, 0, 88, 72, AREA)], [(86, 288, 0, 0, 88, 72, AREA)], [(352, 288, 0, 0, 88, 72, 2)],
                [(352, 288, 0, 0, 2, 72, AREA)], [tiles[0]] * 17):
        ta = api.tiles_array(bad)
        assert lib.vp8hip_set_canvas(hip.h, C.addressof(ta), len(bad), *bg) == ERR_ARG, bad
    ta = api.tiles_array(tiles)
    assert lib.vp8hip_set_canvas(hip.h, C.addressof(ta), 4, 256, 0, 0) == ERR_ARG
    assert lib.vp8hip_set_canvas(hip.h, C.addressof(ta), -1, *bg) == ERR_ARG and lib.vp8hip_set_canvas(hip.h, None, 4, *bg) == ERR_ARG
    unchanged("after invalid canvases")
    # what a canvas excludes, refused by its own setter while the canvas is in force
    pitch = (C.c_int32 * 3)(200, 100, 100)
    assert lib.vp8hip_set_source_scaling(hip.h, 352, 288, 176, 144, 0) == ERR_ARG
    assert lib.vp8hip_set_source_format(hip.h, api.FORMAT_NV12) == ERR_ARG
    assert lib.vp8hip_set_source_window(hip.h, pitch, 0, 0) == ERR_ARG
    assert lib.vp8hip_set_source_orientation(hip.h, 2, 0) == ERR_ARG and lib.vp8hip_set_source_orientation(hip.h, 0, 1) == ERR_ARG
    assert lib.vp8hip_set_deinterlace(hip.h, 1, 0) == ERR_ARG
    unchanged("after the excluded setters")
    # the single-source ways in, hidden frames, a split, a batch
    y, u, v = random_frame(*coded, 74)
    d = [api.to_device(p) for p in (y, u, v)]
    assert lib.vp8hip_set_current_device(hip.h, *[b.data_ptr() for b in d]) == ERR_STATE
    assert lib.vp8hip_upload_current(hip.h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == ERR_STATE
    assert lib.vp8hip_prefetch_current(hip.h, y.ctypes.data, u.ctypes.data, v.ctypes.data) == ERR_STATE
    window = (vp * 3)(*[b.data_ptr() for b in d])
    assert lib.vp8hip_arf_filter_device(hip.h, window, 1, 0, 3) == ERR_ARG
    assert lib.vp8hip_shard_init(hip.h, (C.c_uint8 * 128)(), 0, 1) == ERR_STATE
    other = api.Vp8Hip(*coded)
    pair, out = (vp * 2)(hip.h, other.h), vp()
    assert lib.vp8hip_batch_create(C.byref(out), pair, 2) == ERR_ARG and not out.value
    other.set_canvas(tiles, bg)      # (equal settings are no excuse)
    assert lib.vp8hip_batch_create(C.byref(out), pair, 2) == ERR_ARG and not out.value
    # a frame with a plane missing or a pitch too small
    src, keep = place(frames, False, False)
    for k, entry in ((0, (src[0][0], 0, src[0][2], (0, 0, 0))), (3, (src[3][0], src[3][1], src[3][2], (350, 0, 0))), (2, (src[2][0], src[2][1], src[2][2], (0, 0, 175)))):
        pa, _ = api.tile_planes_array(src[:k] + [entry] + src[k + 1:], 4)
        assert lib.vp8hip_compose_current_host(hip.h, C.addressof(pa)) == ERR_ARG, k
    assert lib.vp8hip_compose_current_host(hip.h, None) == ERR_ARG
    unchanged("after the refused ways in")
    # the other way round: with each of them in force a canvas is refused, and without a canvas the compose calls are
    hip.set_canvas([])
    pa, _ = api.tile_planes_array(src, 4)
    assert lib.vp8hip_compose_current_host(hip.h, C.addressof(pa)) == ERR_STATE and lib.vp8hip_compose_current_device(hip.h, C.addressof(pa)) == ERR_STATE
    for on, off in ((lambda: lib.vp8hip_set_source_scaling(hip.h, 352, 288, 176, 144, 0), lambda: lib.vp8hip_set_source_scaling(hip.h, 0, 0, 0, 0, 0)),
                    (lambda: lib.vp8hip_set_source_format(hip.h, api.FORMAT_NV12), lambda: lib.vp8hip_set_source_format(hip.h, 0)),
                    (lambda: lib.vp8hip_set_source_window(hip.h, pitch, 0, 0), lambda: lib.vp8hip_set_source_window(hip.h, None, 0, 0)),
                    (lambda: lib.vp8hip_set_source_orientation(hip.h, 2, 1), lambda: lib.vp8hip_set_source_orientation(hip.h, 0, 0)),
                    (lambda: lib.vp8hip_set_deinterlace(hip.h, 2, 1), lambda: lib.vp8hip_set_deinterlace(hip.h, 0, 0))):
        assert on() == 0
        assert lib.vp8hip_set_canvas(hip.h, C.addressof(ta), 4, *bg) == ERR_ARG and lib.vp8hip_canvas_tiles(hip.h) == 0
        assert off() == 0
    hip.upload_current(y, u, v)
    assert_surfaces(current_surfaces(hip), (y, u, v), "no canvas: a plain upload")
    hip.set_canvas(tiles, bg)
    unchanged("the canvas again")
    del keep
    for b in d:
        b.free()
    other.close()
    hip.close()


def test_the_drivers_refusals():
    from vp8oclenc_amd import api
    name = "grid_area"
    coded, _, tiles, bg, _ = R.CASES[name]
    frames = R.case_frames(name)
    y, u, v = random_frame(*coded, 75)
    drv = api.NativeDriver(*coded, gop_size=3)
    lib, vp = drv.lib, C.c_void_p
    for fn in ("vp8drv_encode_frame_device", "vp8drv_encode_frame_host"):
        getattr(lib, fn).argtypes = [vp] * 4 + [C.c_int]
    for fn in ("vp8drv_prefetch_frame_host", "vp8drv_stage_frame_host"):
        getattr(lib, fn).argtypes = [vp] * 4
    for fn in ("vp8drv_encode_frame_tiles_device", "vp8drv_encode_frame_tiles_host"):
        getattr(lib, fn).argtypes = [vp, vp, C.c_int]
    lib.vp8drv_set_arf.argtypes = [vp, C.c_int]
    src, keep = place(frames, False, False)
    pa, _ = api.tile_planes_array(src, 4)
    host = (y.ctypes.data, u.ctypes.data, v.ctypes.data)
    assert lib.vp8drv_encode_frame_tiles_host(drv.h, C.addressof(pa), 0) == ERR_STATE and lib.vp8drv_encode_frame_tiles_device(drv.h, C.addressof(pa), 0) == ERR_STATE
    drv.set_canvas(tiles, bg)
    assert lib.vp8drv_encode_frame_host(drv.h, *host, 0) == ERR_STATE and lib.vp8drv_encode_frame_device(drv.h, *host, 0) == ERR_STATE
    assert lib.vp8drv_prefetch_frame_host(drv.h, *host) == ERR_STATE and lib.vp8drv_stage_frame_host(drv.h, *host) == ERR_STATE
    assert lib.vp8drv_set_arf(drv.h, 4) == ERR_STATE
    twin = api.NativeDriver(*coded, gop_size=3)
    twin.set_canvas(tiles, bg)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch([drv, twin])
    twin.close()
    # nothing has changed: the schedule has not moved, and the frames are those of a driver that was never asked
    fresh = api.NativeDriver(*coded, gop_size=3)
    fresh.set_canvas(tiles, bg)
    for t in range(2):
        for d in (drv, fresh):
            d.encode_tiles(src)
        assert drv.get_frame() == fresh.get_frame(), t
    assert drv.stats().frame_number == fresh.stats().frame_number == 2
    fresh.close()
    drv.close()
    del keep
    with pytest.raises(api.Vp8HipError):
        d0 = api.NativeDriver(*coded, device_params=0)
        try:
            d0.set_canvas(tiles, bg)
        finally:
            d0.close()


# ---- 4. the tool ---------------------------------------------------------------------------------------------------------------------------
def test_encode_ivf_canvas_equals_the_drivers_frames(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import decode_ivf
    from vp8oclenc_amd import api
    name = "letterbox_ab"
    coded, (pw, ph), tiles, bg, _ = R.CASES[name]
    n = 4
    seqs = tile_sequences(tiles, n, seed=81)
    seqs[1] = seqs[1][:3]      # the second file ends early: its tile is absent in the last frame
    args = []
    for k, (t, s) in enumerate(zip(tiles, seqs)):
        path = tmp_path / f"tile{k}.yuv"
        path.write_bytes(b"".join(p.tobytes() for f in s for p in f))
        args += ["--tile", f"{path}:{t[0]}x{t[1]}:{t[2]}:{t[3]}:{t[4]}:{t[5]}:{'lanczos' if t[6] else 'area'}"]
    out = tmp_path / "canvas.ivf"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(out), "--canvas", "--width", str(pw), "--height", str(ph), "--frames", str(n),
                        "--gop", "3", "--partitions", "2", "--canvas-bg", ",".join(str(x) for x in bg)] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    Wf, Hf, _, _, packets = decode_ivf.read_ivf(str(out))
    assert (Wf, Hf, len(packets)) == (pw, ph, n)
    drv = api.NativeDriver(*coded, src_width=pw, src_height=ph, gop_size=3, num_partitions=2)
    drv.set_canvas(tiles, bg)
    for t in range(n):
        drv.encode_tiles([s[t] if t < len(s) else None for s in seqs])
        assert drv.get_frame() == packets[t], t
    drv.close()
