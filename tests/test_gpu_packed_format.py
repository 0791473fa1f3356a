"""The packed source formats on the device (vp8hip_set_source_format 16 .. 19, vp8hip_set_source_colour, k_convert_packed_b): the kernel
against the numpy restatement of the rule (tests/packed_format_ref.py) bit for bit, in front of the pack and in front of the scaler,
from device and from host memory; and the bit-exact consequence -- a driver fed BGRA or YUY2 frames codes the bytes of a driver fed the
I420 frames the rule makes of them."""
import ctypes as C

import numpy as np
import pytest

import packed_format_ref as P
from test_scale_cpu import AREA, lib_taps, pad_plane, ref_scale_frame

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4


def current_surfaces(hip):
    from vp8oclenc_amd import api
    return (hip.debug(api.DBG_PYRAMID, 3, 0), hip.debug(api.DBG_CURRENT_CHROMA, 0), hip.debug(api.DBG_CURRENT_CHROMA, 1))


def assert_surfaces(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


def padded(frame, Wc, Hc):
    y, u, v = frame
    return pad_plane(y, Wc, Hc), pad_plane(u, Wc // 2, Hc // 2), pad_plane(v, Wc // 2, Hc // 2)


def set_device(hip, frame):
    """the frame (one plane) from device memory: the second and third pointers are never read, the first is passed again"""
    from vp8oclenc_amd import api
    d = api.to_device(frame)
    hip.set_current_device(d.data_ptr(), d.data_ptr(), d.data_ptr())
    hip.synchronize()
    d.free()


# coded size, source size.  34x18: no multiple of a unit of 16 pixels x 2 rows, and padded; 10x6: narrower than a unit; 2x2: one pixel pair;
# 200x120: 13 x 60 = 780 units, several workgroups of 256 with a partial last one
GEOMETRIES = [((48, 32), (34, 18)), ((64, 48), None), ((16, 16), (10, 6)), ((16, 16), (2, 2)), ((208, 128), (200, 120))]


# ---- 1. the kernel against the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coded,src", GEOMETRIES)
@pytest.mark.parametrize("fmt", P.PACKED)
def test_kernel_equals_the_rule_bit_for_bit(fmt, coded, src):
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(*coded)
    w, h = src or coded
    if src:
        hip.set_source_size(*src)
    hip.set_source_format(fmt)
    matrices = P.MATRICES if src == (34, 18) else [P.BT601_LIMITED, P.BT709_FULL]
    for m in matrices:
        hip.set_source_colour(m)
        for i, frame in enumerate(P.frames_for(fmt, w, h)):
            set_device(hip, frame)
            assert_surfaces(current_surfaces(hip), padded(P.convert_ref(fmt, w, h, frame, m), *coded), f"{P.NAMES[fmt]} matrix {m} {w}x{h} in {coded} frame {i}")
    hip.close()


# ---- 2. through the scaler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["format first", "scaling first"])
@pytest.mark.parametrize("fmt", [P.BGRA, P.YUY2])
def test_through_the_scaler(fmt, order):
    from vp8oclenc_amd import api
    W, H, dst = 96, 64, (48, 32)
    hip = api.Vp8Hip(*dst)
    if order == "format first":
        hip.set_source_colour(P.BT709_LIMITED)
        hip.set_source_format(fmt)
        hip.set_source_scaling(W, H, dst[0], dst[1], AREA)
    else:
        hip.set_source_scaling(W, H, dst[0], dst[1], AREA)
        hip.set_source_format(fmt)
        hip.set_source_colour(P.BT709_LIMITED)
    for i, frame in enumerate(P.frames_for(fmt, W, H)[:2]):
        want = ref_scale_frame(*P.convert_ref(fmt, W, H, frame, P.BT709_LIMITED), dst[0], dst[1], AREA, lib_taps)
        if i == 0:
            set_device(hip, frame)
        else:
            hip.upload_current(frame, frame, frame)
        assert_surfaces(current_surfaces(hip), want, f"{P.NAMES[fmt]} scaled, frame {i}")
    hip.close()


# ---- 3. host paths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [P.BGRA, P.YUY2])
def test_host_paths_equal_the_device_path(fmt):
    from vp8oclenc_amd import api
    coded, (w, h) = (48, 32), (34, 18)
    hip = api.Vp8Hip(*coded)
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    hip.set_source_size(w, h)
    hip.set_source_format(fmt)
    hip.set_source_colour(P.BT601_FULL)
    for i, frame in enumerate(P.frames_for(fmt, w, h)):
        set_device(hip, frame)
        device = current_surfaces(hip)
        assert_surfaces(device, padded(P.convert_ref(fmt, w, h, frame, P.BT601_FULL), *coded), f"{P.NAMES[fmt]} device {i}")
        hip.upload_current(frame, frame, frame)
        assert_surfaces(current_surfaces(hip), device, f"{P.NAMES[fmt]} upload {i}")
        # prefetched, the plane in a page-locked block: the other two pointers the first again (i even), or pointers "end to end" behind
        # it, where planes of another format would lie (i odd); neither is read
        hb = api.HostBuffer(frame)
        ptrs = [hb.data_ptr()] * 3 if not i & 1 else [hb.data_ptr(), hb.data_ptr() + frame.size, hb.data_ptr() + frame.size]
        assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
        assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
        assert_surfaces(current_surfaces(hip), device, f"{P.NAMES[fmt]} prefetched {i}")
        hb.free()
    hip.close()


def test_a_prefetch_made_in_the_other_byte_order_or_under_another_matrix_is_not_used():
    """A prefetch stages the plane's raw bytes and the conversion happens at the upload, so the RESULT alone cannot tell a dropped
    prefetch from a kept one.  The page-locked plane is therefore rewritten between the prefetch (waited for) and the upload: a
    prefetch that was dropped copies the plane anew and shows the new bytes, one that was wrongly kept shows the old ones.  The first
    round, without any change of format or matrix, shows that the probe sees a kept prefetch."""
    from vp8oclenc_amd import api
    coded, (w, h) = (48, 32), (34, 18)
    hip = api.Vp8Hip(*coded)
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    hip.set_source_size(w, h)
    old, new = P.frames_for(P.BGRA, w, h)[0], P.frames_for(P.RGBA, w, h)[0]
    assert not np.array_equal(old, new)
    hb = api.HostBuffer(old)
    ptrs = [hb.data_ptr()] * 3

    def round_trip(before, after):
        """prefetch `old` in state `before`, rewrite the plane, switch to state `after`, upload: the surfaces"""
        C.memmove(hb.data_ptr(), old.ctypes.data, old.nbytes)
        hip.set_source_format(before[0])
        hip.set_source_colour(before[1])
        assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
        api.device_synchronize()      # the copy has left the host's plane
        C.memmove(hb.data_ptr(), new.ctypes.data, new.nbytes)
        hip.set_source_format(after[0])
        hip.set_source_colour(after[1])
        assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
        return current_surfaces(hip)

    want = lambda frame, state: padded(P.convert_ref(state[0], w, h, frame, state[1]), *coded)
    same = (P.BGRA, 0)
    assert_surfaces(round_trip(same, same), want(old, same), "a prefetch that still holds is used: the bytes prefetched")
    # BGRA and RGBA planes have the same number of bytes: only the format tells them apart.  Then a change of matrix alone
    for before, after in (((P.BGRA, 0), (P.RGBA, 0)), ((P.RGBA, 0), (P.BGRA, 0)), ((P.BGRA, 0), (P.BGRA, P.BT709_FULL)), ((P.RGBA, 3), (P.RGBA, 1))):
        assert_surfaces(round_trip(before, after), want(new, after), f"{before} prefetched, {after} uploaded: the plane as it is now")
    hb.free()
    hip.close()


# ---- 4. end to end: the bit-exact consequence ----------------------------------------------------------------------------------------------
W, H = 64, 48


@pytest.fixture(scope="module")
def sequence():
    from vp8oclenc_amd.synth import SynthSequence
    seq = SynthSequence(W, H, seed=77)
    return [tuple(np.ascontiguousarray(p[:H >> (i > 0), :W >> (i > 0)]) for i, p in enumerate(seq.frame(t))) for t in range(3)]


@pytest.fixture(scope="module")
def rgb_sequence(sequence):
    """three BGRA frames that look like the sequence (junk in alpha), and the I420 frames the rule makes of them, per matrix"""
    from vp8oclenc_amd import api
    frames = []
    for t, f in enumerate(sequence):
        px = P.rgb_near_i420(P.BGRA, *f).copy()
        px[3::4] = np.random.default_rng(t).integers(0, 256, W * H)
        frames.append(px)
    return frames


def drive(frames, fmt=None, matrix=None, denoise=0, switch=None, **cfg):
    """a driver fed the frames (device memory; one-plane frames pass their pointer three times) -> the frames' bytes.
    switch: {frame number: format} -- the format is set anew in front of that frame"""
    from vp8oclenc_amd import api
    drv = api.NativeDriver(W, H, gop_size=30, check_ssim=1, **cfg)
    if denoise:
        drv.set_denoise(denoise)
    if matrix is not None:
        drv.set_source_colour(matrix)
    if fmt is not None:
        drv.set_source_format(fmt)
    out = []
    for t, f in enumerate(frames):
        if switch and t in switch:
            drv.set_source_format(switch[t])
        planes = [f] if isinstance(f, np.ndarray) else list(f)
        d = [api.to_device(p) for p in planes]
        ptrs = [b.data_ptr() for b in d]
        key = drv.encode_frame_device(*(ptrs + [ptrs[-1]] * (3 - len(ptrs))))
        assert key == (t == 0)
        out.append(drv.get_frame())
        for b in d:
            b.free()
    drv.close()
    return out


@pytest.mark.parametrize("denoise", [0, 2])
def test_a_driver_fed_bgra_codes_the_bytes_of_a_driver_fed_the_rules_i420(rgb_sequence, denoise):
    want = drive([P.convert_ref(P.BGRA, W, H, f, 0) for f in rgb_sequence], denoise=denoise)      # never told about formats
    assert not (want[0][0] & 1) and (want[1][0] & 1) and (want[2][0] & 1)      # a key frame and two inter frames
    got = drive(rgb_sequence, P.BGRA, denoise=denoise)
    assert got == want, [len(a) == len(b) for a, b in zip(got, want)]


def test_a_driver_fed_yuy2_made_from_i420_codes_the_i420_drivers_bytes(sequence):
    want = drive(sequence)
    for fmt in (P.YUY2, P.UYVY):
        assert drive([P.from_i420(fmt, *f) for f in sequence], fmt) == want, P.NAMES[fmt]


def test_grey_bgra_at_full_range_codes_the_bytes_of_the_grey_i420_frames(sequence):
    grey = [(f[0], np.full_like(f[1], 128), np.full_like(f[2], 128)) for f in sequence]
    want = drive(grey)
    assert drive([P.grey_rgb(P.BGRA, f[0]) for f in sequence], P.BGRA, matrix=P.BT601_FULL) == want


# ---- 5. off is off ------------------------------------------------------------------------------------------------------------------------
def test_off_is_off(sequence, rgb_sequence):
    want = drive(sequence)
    for m in P.MATRICES:
        assert drive(sequence, matrix=m) == want, m      # a matrix with format 0 changes no byte
    # format 18 then 0 between frames: a correct I420 intake again
    i420 = [P.convert_ref(P.BGRA, W, H, f, 0) for f in rgb_sequence]
    assert drive([rgb_sequence[0], i420[1], i420[2]], P.BGRA, switch={1: 0}) == drive(i420)
    assert drive([i420[0], rgb_sequence[1], i420[2]], switch={1: P.BGRA, 2: 0}) == drive(i420)


# ---- 6. batches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_a_batch_of_two_equals_the_two_alone(rgb_sequence, host):
    from vp8oclenc_amd import api
    fmt, m = P.BGRA, P.BT709_LIMITED
    seqs = [rgb_sequence, rgb_sequence[::-1]]
    alone = [drive(s, fmt, matrix=m) for s in seqs]
    assert alone[0] == drive([P.convert_ref(fmt, W, H, f, m) for f in seqs[0]])      # (and those are the I420 driver's bytes)
    drvs = [api.NativeDriver(W, H, gop_size=30, check_ssim=1) for _ in seqs]
    for d in drvs:
        d.set_source_format(fmt)
        d.set_source_colour(m)
    batch = api.NativeBatch(drvs)
    lib = drvs[0].lib
    lib.vp8drv_set_source_colour.argtypes = [C.c_void_p, C.c_int]
    assert lib.vp8drv_set_source_colour(drvs[0].h, 0) == ERR_STATE      # a member of a live batch
    for t in range(3):
        make = api.HostBuffer if host else api.to_device
        bufs = [make(s[t]) for s in seqs]
        batch.encode_frame_device([(b.data_ptr(),) * 3 for b in bufs], host=host)
        for i, d in enumerate(drvs):
            assert d.get_frame() == alone[i][t], (t, i)
        for b in bufs:
            b.free()
    batch.close()
    assert lib.vp8drv_set_source_colour(drvs[0].h, 0) == 0              # ... and free again
    for d in drvs:
        d.close()


def test_members_that_disagree_on_the_matrix_make_no_batch():
    from vp8oclenc_amd import api
    odd = [api.NativeDriver(W, H), api.NativeDriver(W, H)]
    for d in odd:
        d.set_source_format(P.BGRA)
    odd[1].set_source_colour(P.BT709_LIMITED)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(odd)
    odd[0].set_source_colour("bt709", "limited")
    api.NativeBatch(odd).close()
    for d in odd:
        d.close()
    # the library's own check, under the driver's
    ctx = [api.Vp8Hip(W, H), api.Vp8Hip(W, H)]
    for c in ctx:
        c.set_source_format(P.RGBA)
    ctx[0].set_source_colour(P.BT601_FULL)
    lib = ctx[0].lib
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(h), (C.c_void_p * 2)(ctx[0].h, ctx[1].h), 2) == ERR_ARG
    ctx[1].set_source_colour(P.BT601_FULL)
    assert lib.vp8hip_batch_create(C.byref(h), (C.c_void_p * 2)(ctx[0].h, ctx[1].h), 2) == 0
    lib.vp8hip_batch_destroy(h)
    for c in ctx:
        c.close()


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(W, H)
    lib = hip.lib
    for f in (lib.vp8hip_set_source_format, lib.vp8drv_set_source_format, lib.vp8hip_set_source_colour, lib.vp8drv_set_source_colour):
        f.argtypes = [C.c_void_p, C.c_int]
    for bad in list(range(8, 16)) + [20, -1, 1 << 20]:
        assert lib.vp8hip_set_source_format(hip.h, bad) == ERR_ARG, bad
    for bad in (4, -1, 1 << 20):
        assert lib.vp8hip_set_source_colour(hip.h, bad) == ERR_ARG, bad
    assert lib.vp8hip_set_source_colour(None, 0) == ERR_ARG
    with pytest.raises(api.Vp8HipError) as e:
        hip.set_source_colour(4)
    assert e.value.args[1] == ERR_ARG
    with pytest.raises(ValueError):
        hip.set_source_colour("bt2020")
    with pytest.raises(ValueError):
        hip.set_source_format("rgb24")
    with pytest.raises(ValueError):
        api.source_format(8)
    # refused: the context still takes I420
    rng = np.random.default_rng(1)
    f = (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8),
         rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8))
    hip.upload_current(*f)
    assert_surfaces(current_surfaces(hip), f, "after refusals")
    # the names
    hip.set_source_format("bgra")
    hip.set_source_colour("bt709", "full")
    frame = P.frames_for(P.BGRA, W, H)[0]
    hip.upload_current(frame, frame, frame)
    assert_surfaces(current_surfaces(hip), P.convert_ref(P.BGRA, W, H, frame, P.BT709_FULL), "by name")
    hip.close()
    drv = api.NativeDriver(W, H)
    for bad in list(range(8, 16)) + [20, -1]:
        assert lib.vp8drv_set_source_format(drv.h, bad) == ERR_ARG
    for bad in (4, -1):
        assert lib.vp8drv_set_source_colour(drv.h, bad) == ERR_ARG
    assert lib.vp8drv_set_source_colour(None, 0) == ERR_ARG
    with pytest.raises(api.Vp8HipError) as e:
        drv.set_source_colour(7)
    assert e.value.args[1] == ERR_ARG
    drv.encode_frame_host(*f)      # ... and the driver still takes I420
    assert len(drv.get_frame()) > 10
    drv.close()
    host_params = api.NativeDriver(W, H, device_params=0)
    assert lib.vp8drv_set_source_format(host_params.h, P.BGRA) == ERR_ARG
    assert lib.vp8drv_set_source_colour(host_params.h, 1) == ERR_ARG
    with pytest.raises(api.Vp8HipError) as e:
        host_params.set_source_colour("bt709")
    assert e.value.args[1] == ERR_ARG
    host_params.close()


# ---- 8. the tools -------------------------------------------------------------------------------------------------------------------------
def test_encode_ivf_takes_a_raw_bgra_file(tmp_path, rgb_sequence):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    np.concatenate(rgb_sequence).tofile(tmp_path / "in.bgra")
    for name, m in (("m0", 0), ("m3", P.BT709_FULL)):
        np.concatenate([np.concatenate([p.ravel() for p in P.convert_ref(P.BGRA, W, H, f, m)]) for f in rgb_sequence]).tofile(tmp_path / f"{name}.yuv")

    def py(src, out, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "encode_ivf.py"), str(tmp_path / out), "--yuv", str(tmp_path / src), "--width", str(W),
                            "--height", str(H), "--gop", "3"] + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read()
    assert py("in.bgra", "a.ivf", "--source-format", "bgra") == py("m0.yuv", "a_direct.ivf")
    assert py("in.bgra", "b.ivf", "--source-format", "bgra", "--source-matrix", "bt709", "--source-range", "full") == py("m3.yuv", "b_direct.ivf")
