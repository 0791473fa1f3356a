"""HDR tone mapping on the device (vp8hip_set_source_transfer, k_tonemap_b) through the C ABI: the kernel against the rule in plain C++
(vp8host_tonemap_frame, which tests/test_tonemap_cpu.py holds to the numpy restatement) byte for byte, every route a frame becomes
current by, one composition with the window and the scaler, the bit-exact consequence at driver level -- a driver fed P010 PQ frames
codes the bytes of an I420 driver fed the mapped frames -- the setters' rules, and the native tool's option."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import tonemap_ref as T
from test_scale_cpu import AREA, lib_taps, pad_plane, ref_scale_frame

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(T.PQ, 1000), (T.PQ, 10000), (T.HLG, 1000)]
MATRICES = [0, 3]
# narrower than a lane's unit of 16 pixels; a last unit that is moved left; several workgroups and a ragged edge
SIZES = [(2, 2), (6, 4), (18, 10), (34, 6), (130, 66)]


def current_surfaces(hip):
    from vp8oclenc_amd import api
    return (hip.debug(api.DBG_PYRAMID, 3, 0), hip.debug(api.DBG_CURRENT_CHROMA, 0), hip.debug(api.DBG_CURRENT_CHROMA, 1))


def assert_surfaces(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


def coded_size(w, h):
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


def padded(frame, Wc, Hc):
    y, u, v = frame
    return pad_plane(y, Wc, Hc), pad_plane(u, Wc // 2, Hc // 2), pad_plane(v, Wc // 2, Hc // 2)


def three(ptrs):
    """the three pointers of a call: P010 passes the second again"""
    return list(ptrs) + [ptrs[1]] * (3 - len(ptrs))


def context(fmt, w, h, transfer=None, peak=1000, matrix=0):
    from vp8oclenc_amd import api
    coded = coded_size(w, h)
    hip = api.Vp8Hip(*coded)
    if coded != (w, h):
        hip.set_source_size(w, h)
    hip.set_source_format(fmt)
    hip.set_source_colour(matrix)
    if transfer:
        hip.set_source_transfer(transfer, peak)
    return hip, coded


def take_device(hip, planes):
    from vp8oclenc_amd import api
    d = [api.to_device(p) for p in planes]
    hip.set_current_device(*three([b.data_ptr() for b in d]))
    hip.synchronize()
    out = current_surfaces(hip)
    for b in d:
        b.free()
    return out


# ---- 1. the kernel against the rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fmt", [T.P010, T.I010])
def test_kernel_equals_the_rule_byte_for_byte(fmt, size):
    from vp8oclenc_amd import api
    w, h = size
    hip, coded = context(fmt, w, h)
    frames = [(name, T.make_planes(fmt, y, cb, cr, junk=41)) for name, y, cb, cr in T.inputs(w, h)]
    for transfer, peak in PAIRS:
        for matrix in MATRICES:
            hip.set_source_colour(matrix)
            hip.set_source_transfer(transfer, peak)
            for name, planes in frames:
                want = api.tonemap_frame(fmt, transfer, peak, w, h, planes, matrix)
                assert_surfaces(take_device(hip, planes), padded(want, *coded), f"format {fmt} {w}x{h} transfer {transfer}:{peak} matrix {matrix} {name}")
    hip.close()


def test_kernel_equals_the_rule_at_1920x1080():
    from vp8oclenc_amd import api
    w, h = 1920, 1080
    rng = np.random.default_rng(11)
    y, cb, cr = rng.integers(0, 1024, (h, w)), rng.integers(0, 1024, (h // 2, w // 2)), rng.integers(0, 1024, (h // 2, w // 2))
    y[: h // 2] = np.linspace(0, 1023, (h // 2) * w).reshape(h // 2, w)      # the upper half: a ramp under random chroma
    planes = T.make_planes(T.P010, y, cb, cr)
    hip, coded = context(T.P010, w, h, T.PQ, 1000, 1)
    assert_surfaces(take_device(hip, planes), padded(api.tonemap_frame(T.P010, T.PQ, 1000, w, h, planes, 1), *coded), "P010 1920x1080 PQ 1000")
    hip.close()


# ---- 2. every route gives the same bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [T.P010, T.I010])
def test_every_route_gives_the_same_bytes(fmt):
    from vp8oclenc_amd import api
    w, h = 34, 18
    frames = [T.make_planes(fmt, *T.inputs(w, h, seed=s)[0][1:]) for s in (1, 2, 3)]
    want = [padded(api.tonemap_frame(fmt, T.HLG, 1000, w, h, f, 0), *coded_size(w, h)) for f in frames]
    hip, _ = context(fmt, w, h, T.HLG, 1000)
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    assert_surfaces(take_device(hip, frames[0]), want[0], "set_current_device")
    hip.upload_current(*three(frames[1]))
    assert_surfaces(current_surfaces(hip), want[1], "upload_current")
    hb = [api.HostBuffer(p) for p in frames[2]]
    ptrs = three([b.data_ptr() for b in hb])
    assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
    assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
    assert_surfaces(current_surfaces(hip), want[2], "prefetch_current, then upload_current")
    # a prefetch made under another peak is dropped: the planes are copied again and mapped at the peak in force
    assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
    hip.set_source_transfer(T.HLG, 400)
    assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
    assert_surfaces(current_surfaces(hip), padded(api.tonemap_frame(fmt, T.HLG, 400, w, h, frames[2], 0), *coded_size(w, h)), "after a stale prefetch")
    for b in hb:
        b.free()
    hip.close()
    # a batch of three members with different frames: blockIdx.z is the member
    members = [context(fmt, w, h, T.HLG, 1000)[0] for _ in range(3)]
    arr = C.POINTER(C.c_void_p)
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), arr, C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    lib.vp8hip_batch_set_current_device.argtypes = [C.c_void_p, C.POINTER(C.c_int), arr, arr, arr]
    batch = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(batch), (C.c_void_p * 3)(*[m.h for m in members]), 3) == 0
    dev = [[api.to_device(p) for p in f] for f in frames]
    plane = lambda k: (C.c_void_p * 3)(*[d[min(k, len(d) - 1)].data_ptr() for d in dev])
    assert lib.vp8hip_batch_set_current_device(batch, None, plane(0), plane(1), plane(2)) == 0
    for i, m in enumerate(members):
        m.synchronize()
        assert_surfaces(current_surfaces(m), want[i], f"batch member {i}")
    lib.vp8hip_batch_destroy(batch)
    for m in members:
        m.close()
    for d in dev:
        for b in d:
            b.free()


# ---- 3. one composition: window, tone mapping, scaler ----------------------------------------------------------------------------------
def test_window_tonemap_and_scaler_compose_in_take_frames_order():
    from vp8oclenc_amd import api
    W, H, dst, (x, y) = 96, 64, (48, 32), (8, 6)
    pitch = [300, 300, 0]      # a P010 surface of 128 x 80: 256 bytes a row in both planes, pitched to 300
    rng = np.random.default_rng(21)
    surface = [rng.integers(0, 256, (80, 300), dtype=np.uint8), rng.integers(0, 256, (40, 300), dtype=np.uint8)]
    hip = api.Vp8Hip(*dst)
    hip.set_source_format(T.P010)
    hip.set_source_scaling(W, H, dst[0], dst[1], AREA)
    hip.set_source_window(pitch, x, y)
    hip.set_source_transfer(T.PQ, 4000)
    hip.set_source_colour(1)
    window = api.window_frame(T.P010, W, H, x, y, pitch, surface)
    mapped = api.tonemap_frame(T.P010, T.PQ, 4000, W, H, window, 1)
    want = ref_scale_frame(*mapped, dst[0], dst[1], AREA, lib_taps)
    assert_surfaces(take_device(hip, surface), want, "window + tone mapping + 2:1 area scaling, device")
    hip.upload_current(*three(surface))
    assert_surfaces(current_surfaces(hip), want, "... from the host")
    hip.close()


# ---- 4. the bit-exact consequence at driver level ----------------------------------------------------------------------------------------
W, H, FRAMES = 64, 48, 6


@pytest.fixture(scope="module")
def videos():
    """three videos of six P010 frames (a moving synthetic picture's codes, shifted up to ten bits: a valid PQ signal) and the I420
    frames vp8host_tonemap_frame makes of them at (PQ, 1000), matrix 0"""
    from vp8oclenc_amd import api
    from vp8oclenc_amd.synth import SynthSequence
    out = []
    for seed in (77, 78, 79):
        seq = SynthSequence(W, H, seed=seed)
        hdr = [api.planes_from_i420(T.P010, *[np.ascontiguousarray(p[:H >> (i > 0), :W >> (i > 0)]) for i, p in enumerate(seq.frame(t))]) for t in range(FRAMES)]
        out.append((hdr, [api.tonemap_frame(T.P010, T.PQ, 1000, W, H, f, 0) for f in hdr]))
    return out


def drive_alone(frames, fmt=0, transfer=0):
    from vp8oclenc_amd import api
    drv = api.NativeDriver(W, H, gop_size=4, check_ssim=1)
    if transfer:
        drv.set_source_transfer(transfer, 1000)      # (before the format: the order does not matter)
    if fmt:
        drv.set_source_format(fmt)
    out = []
    for t, f in enumerate(frames):
        d = [api.to_device(np.ascontiguousarray(p)) for p in f]
        drv.encode_frame_device(*three([b.data_ptr() for b in d]))
        out.append(drv.get_frame())
        for b in d:
            b.free()
    drv.close()
    return out


def drive_batch(videos_frames, transfer):
    from vp8oclenc_amd import api
    drvs = [api.NativeDriver(W, H, gop_size=4, check_ssim=1) for _ in videos_frames]
    for d in drvs:
        if transfer:
            d.set_source_format(T.P010)
            d.set_source_transfer(T.PQ, 1000)
    batch = api.NativeBatch(drvs)
    out = [[] for _ in drvs]
    for t in range(FRAMES):
        dev = [[api.to_device(np.ascontiguousarray(p)) for p in v[t]] for v in videos_frames]
        batch.encode_frame_device([tuple(three([b.data_ptr() for b in d])) for d in dev])
        for i, d in enumerate(drvs):
            out[i].append(d.get_frame())
        for d in dev:
            for b in d:
                b.free()
    batch.close()
    for d in drvs:
        d.close()
    return out


def test_a_driver_fed_pq_frames_codes_the_bytes_of_the_mapped_i420_frames(videos):
    hdr, sdr = videos[0]
    want = drive_alone(sdr)
    kinds = [f[0] & 1 for f in want]
    assert kinds[0] == 0 and 0 in kinds[1:] and 1 in kinds      # the first key frame, one inside the run, and inter frames
    assert drive_alone(hdr, T.P010, T.PQ) == want
    assert drive_alone(hdr, T.P010) != want                      # (and without the transfer the picture is another one)


def test_a_batch_of_three_codes_the_bytes_of_the_mapped_i420_frames(videos):
    want = drive_batch([sdr for _, sdr in videos], False)
    assert want[0] != want[1] != want[2]
    assert drive_batch([hdr for hdr, _ in videos], True) == want


# ---- 5. the setters' rules -----------------------------------------------------------------------------------------------------------------
def test_setter_rules():
    from vp8oclenc_amd import api
    w, h = 34, 18
    _, y, cb, cr = T.inputs(w, h)[0]
    planes = T.make_planes(T.I010, y, cb, cr, junk=13)
    want = padded(api.tonemap_frame(T.I010, T.HLG, 1000, w, h, planes, 0), *coded_size(w, h))
    # the order of the two setters does not matter
    for order in ("format first", "transfer first"):
        hip = api.Vp8Hip(*coded_size(w, h))
        hip.set_source_size(w, h)
        for step in (("f", "t") if order == "format first" else ("t", "f")):
            hip.set_source_format(T.I010) if step == "f" else hip.set_source_transfer(T.HLG, 1000)
        assert_surfaces(take_device(hip, planes), want, order)
        lib = hip.lib
        lib.vp8hip_set_source_format.argtypes = [C.c_void_p, C.c_int]
        lib.vp8hip_set_source_transfer.argtypes = [C.c_void_p, C.c_int, C.c_int]
        # what the rule does not cover is refused by whichever setter would complete it, and changes nothing
        for fmt in (6, 7, 1, 16):
            assert lib.vp8hip_set_source_format(hip.h, fmt) == ERR_ARG, fmt
        for transfer, peak in ((T.HLG, 399), (T.PQ, 10001), (3, 1000), (-1, 1000)):
            assert lib.vp8hip_set_source_transfer(hip.h, transfer, peak) == ERR_ARG, (transfer, peak)
        assert lib.vp8hip_set_source_transfer(None, T.PQ, 1000) == ERR_ARG
        assert_surfaces(take_device(hip, planes), want, order + ", after refusals")
        # off again: today's k_convert_b bytes
        hip.set_source_transfer(0, 0)
        plain = (np.minimum(255, (y + 2) >> 2).astype(np.uint8), np.minimum(255, (cb + 2) >> 2).astype(np.uint8), np.minimum(255, (cr + 2) >> 2).astype(np.uint8))
        assert_surfaces(take_device(hip, planes), padded(plain, *coded_size(w, h)), order + ", transfer 0 afterwards")
        for fmt in (6, 7, 1, 16):      # ... and with those formats in force the transfer is refused, and the format stays
            assert lib.vp8hip_set_source_format(hip.h, fmt) == 0, fmt
            assert lib.vp8hip_set_source_transfer(hip.h, T.PQ, 1000) == ERR_ARG, fmt
            assert lib.vp8hip_set_source_transfer(hip.h, 0, 0) == 0
        hip.close()


def test_members_that_disagree_make_no_batch():
    from vp8oclenc_amd import api
    drvs = [api.NativeDriver(W, H), api.NativeDriver(W, H)]
    for d in drvs:
        d.set_source_format(T.P010)
    drvs[0].set_source_transfer(T.PQ, 1000)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(drvs)                      # one maps, one does not
    drvs[1].set_source_transfer(T.HLG, 1000)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(drvs)                      # two transfers
    drvs[1].set_source_transfer(T.PQ, 4000)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(drvs)                      # two peaks
    drvs[1].set_source_transfer(T.PQ, 1000)
    batch = api.NativeBatch(drvs)
    lib = drvs[0].lib
    lib.vp8drv_set_source_transfer.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert lib.vp8drv_set_source_transfer(drvs[0].h, 0, 0) == ERR_STATE      # a member of a live batch
    batch.close()
    assert lib.vp8drv_set_source_transfer(drvs[0].h, 0, 0) == 0
    for bad in ((3, 1000), (T.PQ, 399)):
        assert lib.vp8drv_set_source_transfer(drvs[0].h, *bad) == ERR_ARG
    for d in drvs:
        d.close()
    host_params = api.NativeDriver(W, H, device_params=0)
    assert lib.vp8drv_set_source_transfer(host_params.h, T.PQ, 1000) == ERR_ARG
    host_params.close()
    # the library's own check, under the driver's
    ctx = [api.Vp8Hip(W, H), api.Vp8Hip(W, H)]
    for c in ctx:
        c.set_source_format(T.I010)
        c.set_source_transfer(T.PQ, 1000)
    ctx[1].set_source_transfer(T.PQ, 1001)
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    h = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(h), (C.c_void_p * 2)(ctx[0].h, ctx[1].h), 2) == ERR_ARG
    for c in ctx:
        c.close()


# ---- 6. the native tool -----------------------------------------------------------------------------------------------------------------------
def test_the_tool_maps_a_c420p10_file_and_refuses_an_8_bit_one(tmp_path):
    from vp8oclenc_amd import api, y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "y4m_to_ivf")
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", "y4m_to_ivf.cpp"), "-o", exe,
                    "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    from vp8oclenc_amd.synth import SynthSequence
    seq = SynthSequence(W, H, seed=5)
    sdr = [[np.ascontiguousarray(p[:H >> (i > 0), :W >> (i > 0)]) for i, p in enumerate(seq.frame(t))] for t in range(5)]
    hdr = [api.planes_from_i420(T.I010, *f) for f in sdr]
    y4m.write_y4m(str(tmp_path / "hlg.y4m"), hdr, framerate=25, tag="C420p10", size=(W, H))
    y4m.write_y4m(str(tmp_path / "mapped.y4m"), [api.tonemap_frame(T.I010, T.HLG, 1000, W, H, f, 0) for f in hdr], framerate=25)
    y4m.write_y4m(str(tmp_path / "sdr.y4m"), sdr, framerate=25)

    def run(src, out, *extra, ok=True):
        r = subprocess.run([exe, str(tmp_path / src), str(tmp_path / out), "-g", "3"] + list(extra), capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read() if ok else r.stderr
    mapped = run("mapped.y4m", "mapped.ivf")
    assert run("hlg.y4m", "hlg.ivf", "-input-transfer", "hlg") == mapped
    assert run("hlg.y4m", "hlg1000.ivf", "-input-transfer", "hlg:1000") == mapped
    assert run("hlg.y4m", "hlg400.ivf", "-input-transfer", "hlg:400") != mapped
    assert run("hlg.y4m", "plain.ivf") != mapped
    err = run("sdr.y4m", "no.ivf", "-input-transfer", "hlg", ok=False)
    assert "-input-transfer" in err and "C420jpeg" in err
    assert "-input-transfer" in run("hlg.y4m", "no.ivf", "-input-transfer", "hlg:99", ok=False)
