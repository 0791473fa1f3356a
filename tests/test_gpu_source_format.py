"""Source formats on the device (vp8hip_set_source_format, k_convert_b): the kernel against the numpy restatement of the rule
(tests/source_format_ref.py) bit for bit, in front of the pack and in front of the scaler, from device and from host memory; and its
bit-exact consequence -- a driver fed NV12, P010 or 4:4:4 planes of a frame codes the bytes of a driver fed that frame as I420."""
import ctypes as C

import numpy as np
import pytest

import source_format_ref as R
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


def three(ptrs):
    """the three pointers of a call: the two-plane formats pass the second again"""
    return list(ptrs) + [ptrs[1]] * (3 - len(ptrs))


def frames_for(fmt, w, h):
    """random samples with junk in the bits that carry no value, and the extremes: all-maximum (the clamp at ten bits) and all-zero"""
    shapes = [(h, w), R.chroma_shape(fmt, w, h), R.chroma_shape(fmt, w, h)]
    junk = np.random.default_rng(9).integers(0, 64, (h, w))
    return [R.make_planes(fmt, *R.random_samples(fmt, w, h, 100 + fmt), junk=junk),
            R.make_planes(fmt, *[np.full(s, R.max_sample(fmt)) for s in shapes]),
            R.make_planes(fmt, *[np.zeros(s, np.int32) for s in shapes]),
            R.make_planes(fmt, *R.random_samples(fmt, w, h, 200 + fmt))]


# coded size, source size: 34x18 is no multiple of a vector width (chroma 17 wide) and is padded by 14 and 14; 64x48 has no source size;
# 10x6 in 16x16 is narrower than a vector, in luma and in chroma
GEOMETRIES = [((48, 32), (34, 18)), ((64, 48), None), ((16, 16), (10, 6))]


# ---- 1. the kernel against the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coded,src", GEOMETRIES)
@pytest.mark.parametrize("fmt", R.CONVERTED)
def test_kernel_equals_the_rule_bit_for_bit(fmt, coded, src):
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(*coded)
    w, h = src or coded
    if src:
        hip.set_source_size(*src)
    hip.set_source_format(fmt)
    for i, planes in enumerate(frames_for(fmt, w, h)):
        d = [api.to_device(p) for p in planes]
        hip.set_current_device(*three([b.data_ptr() for b in d]))
        hip.synchronize()
        assert_surfaces(current_surfaces(hip), padded(R.convert_ref(fmt, w, h, planes), *coded), f"{R.NAMES[fmt]} {w}x{h} in {coded} frame {i}")
        for b in d:
            b.free()
    hip.close()


# ---- 2. through the scaler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["format first", "scaling first"])
@pytest.mark.parametrize("fmt", [R.NV12, R.I210])
def test_through_the_scaler(fmt, order):
    from vp8oclenc_amd import api
    W, H, dst = 96, 64, (48, 32)
    hip = api.Vp8Hip(*dst)
    if order == "format first":
        hip.set_source_format(fmt)
        hip.set_source_scaling(W, H, dst[0], dst[1], AREA)
    else:
        hip.set_source_scaling(W, H, dst[0], dst[1], AREA)
        hip.set_source_format(fmt)
    for i, planes in enumerate(frames_for(fmt, W, H)[:2]):
        want = ref_scale_frame(*R.convert_ref(fmt, W, H, planes), dst[0], dst[1], AREA, lib_taps)
        if i == 0:
            d = [api.to_device(p) for p in planes]
            hip.set_current_device(*three([b.data_ptr() for b in d]))
            hip.synchronize()
        else:
            hip.upload_current(*three(planes))
        assert_surfaces(current_surfaces(hip), want, f"{R.NAMES[fmt]} scaled, frame {i}")
    hip.close()


# ---- 3. host paths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.NV12, R.P010])
def test_host_paths_equal_the_device_path(fmt):
    from vp8oclenc_amd import api
    coded, (w, h) = (48, 32), (34, 18)
    hip = api.Vp8Hip(*coded)
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    hip.set_source_size(w, h)
    hip.set_source_format(fmt)
    for i, planes in enumerate(frames_for(fmt, w, h)):
        d = [api.to_device(p) for p in planes]
        hip.set_current_device(*three([b.data_ptr() for b in d]))
        hip.synchronize()
        device = current_surfaces(hip)
        assert_surfaces(device, padded(R.convert_ref(fmt, w, h, planes), *coded), f"{R.NAMES[fmt]} device {i}")
        hip.upload_current(*three(planes))
        assert_surfaces(current_surfaces(hip), device, f"{R.NAMES[fmt]} upload {i}")
        # prefetched: planes apart (i even) or end to end in one page-locked block (i odd: one copy)
        if i & 1:
            hb = [api.HostBuffer(np.concatenate(planes))]
            ptrs = [hb[0].data_ptr(), hb[0].data_ptr() + planes[0].size]
        else:
            hb = [api.HostBuffer(p) for p in planes]
            ptrs = [b.data_ptr() for b in hb]
        assert lib.vp8hip_prefetch_current(hip.h, *three(ptrs)) == 0
        assert lib.vp8hip_upload_current(hip.h, *three(ptrs)) == 0
        assert_surfaces(current_surfaces(hip), device, f"{R.NAMES[fmt]} prefetched {i}")
        for b in d + hb:
            b.free()
    # a prefetch made in another format is not used: NV12 and I420 planes have the same number of bytes
    if fmt == R.NV12:
        planes = frames_for(fmt, w, h)[0]
        hb = api.HostBuffer(np.concatenate(planes))
        ptrs = [hb.data_ptr(), hb.data_ptr() + w * h, hb.data_ptr() + w * h + (w // 2) * (h // 2)]
        hip.set_source_format(R.I420)
        assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
        hip.set_source_format(fmt)
        assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
        assert_surfaces(current_surfaces(hip), padded(R.convert_ref(fmt, w, h, planes), *coded), "after a stale prefetch")
        hb.free()
    hip.close()


# ---- 4. end to end: the bit-exact consequence ----------------------------------------------------------------------------------------------
W, H = 64, 48


@pytest.fixture(scope="module")
def sequence():
    from vp8oclenc_amd.synth import SynthSequence
    seq = SynthSequence(W, H, seed=77)
    return [tuple(np.ascontiguousarray(p[:H >> (i > 0), :W >> (i > 0)]) for i, p in enumerate(seq.frame(t))) for t in range(3)]


def drive(frames_of, formats, denoise=0, **cfg):
    """a driver fed frame t as formats[t]'s planes (device memory) -> the frames' bytes; the format is set when it changes"""
    from vp8oclenc_amd import api
    drv = api.NativeDriver(W, H, gop_size=30, check_ssim=1, **cfg)
    if denoise:
        drv.set_denoise(denoise)
    out, now = [], None
    for t, fmt in enumerate(formats):
        if fmt is not None and fmt != now:
            drv.set_source_format(fmt)
            now = fmt
        planes = frames_of(t, fmt or R.I420)
        d = [api.to_device(p) for p in planes]
        key = drv.encode_frame_device(*three([b.data_ptr() for b in d]))
        assert key == (t == 0)
        out.append(drv.get_frame())
        for b in d:
            b.free()
    drv.close()
    return out


@pytest.mark.parametrize("denoise", [0, 2])
def test_a_driver_fed_another_format_codes_the_i420_drivers_bytes(sequence, denoise):
    carried = lambda t, fmt: R.from_i420(fmt, *sequence[t])
    want = drive(carried, [None] * 3, denoise)      # never told about formats
    assert not (want[0][0] & 1) and (want[1][0] & 1) and (want[2][0] & 1)      # a key frame and two inter frames
    for fmt in (R.NV12, R.P010, R.I444):
        got = drive(carried, [fmt] * 3, denoise)
        assert got == want, (R.NAMES[fmt], [len(a) == len(b) for a, b in zip(got, want)])


def test_off_is_off(sequence):
    carried = lambda t, fmt: R.from_i420(fmt, *sequence[t])
    want = drive(carried, [None] * 3)
    assert drive(carried, [R.I420] * 3) == want                 # set to 0: as if never called
    assert drive(carried, [R.NV12, R.I420, R.I420]) == want     # 1 -> 0 between frames: a correct I420 intake again
    assert drive(carried, [R.I420, R.P010, R.I420]) == want


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_a_batch_of_two_equals_the_two_alone(sequence, host):
    from vp8oclenc_amd import api
    fmt = R.NV12
    seqs = [sequence, sequence[::-1]]
    cfg = dict(gop_size=30, check_ssim=1)
    alone = []
    for s in seqs:
        drv = api.NativeDriver(W, H, **cfg)
        drv.set_source_format(fmt)
        out = []
        for f in s:
            d = [api.to_device(p) for p in R.from_i420(fmt, *f)]
            drv.encode_frame_device(*three([b.data_ptr() for b in d]))
            out.append(drv.get_frame())
            for b in d:
                b.free()
        drv.close()
        alone.append(out)
    plain = api.NativeDriver(W, H, **cfg)      # (and those are the I420 driver's bytes)
    for t, f in enumerate(seqs[0]):
        plain.encode_frame_host(*f)
        assert plain.get_frame() == alone[0][t], t
    plain.close()
    drvs = [api.NativeDriver(W, H, **cfg) for _ in seqs]
    for d in drvs:
        d.set_source_format(fmt)
    batch = api.NativeBatch(drvs)
    lib = drvs[0].lib
    lib.vp8drv_set_source_format.argtypes = [C.c_void_p, C.c_int]
    assert lib.vp8drv_set_source_format(drvs[0].h, R.I420) == ERR_STATE      # a member of a live batch
    ny = W * H
    for t in range(3):
        make = api.HostBuffer if host else api.to_device
        bufs = [make(np.concatenate(R.from_i420(fmt, *s[t]))) for s in seqs]
        batch.encode_frame_device([(b.data_ptr(), b.data_ptr() + ny, b.data_ptr() + ny) for b in bufs], host=host)
        for i, d in enumerate(drvs):
            assert d.get_frame() == alone[i][t], (t, i)
        for b in bufs:
            b.free()
    batch.close()
    assert lib.vp8drv_set_source_format(drvs[0].h, R.I420) == 0              # ... and free again
    for d in drvs:
        d.close()


def test_members_that_disagree_on_the_format_make_no_batch():
    from vp8oclenc_amd import api
    odd = [api.NativeDriver(W, H), api.NativeDriver(W, H)]
    odd[1].set_source_format(R.NV12)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(odd)
    odd[0].set_source_format(R.P010)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(odd)
    odd[0].set_source_format(R.NV12)
    api.NativeBatch(odd).close()
    for d in odd:
        d.close()
    # the library's own check, under the driver's
    ctx = [api.Vp8Hip(W, H), api.Vp8Hip(W, H)]
    ctx[0].set_source_format(R.I444)
    lib = ctx[0].lib
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    h = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(h), (C.c_void_p * 2)(ctx[0].h, ctx[1].h), 2) == ERR_ARG
    for c in ctx:
        c.close()


# ---- 6. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(W, H)
    lib = hip.lib
    lib.vp8hip_set_source_format.argtypes = [C.c_void_p, C.c_int]
    lib.vp8drv_set_source_format.argtypes = [C.c_void_p, C.c_int]
    for bad in (8, -1, 1 << 20):
        assert lib.vp8hip_set_source_format(hip.h, bad) == ERR_ARG
    assert lib.vp8hip_set_source_format(None, R.NV12) == ERR_ARG
    # refused: the context still takes I420
    rng = np.random.default_rng(1)
    f = (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8),
         rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8))
    hip.upload_current(*f)
    assert_surfaces(current_surfaces(hip), f, "after refusals")
    hip.close()
    drv = api.NativeDriver(W, H)
    for bad in (8, -1):
        assert lib.vp8drv_set_source_format(drv.h, bad) == ERR_ARG
    assert lib.vp8drv_set_source_format(None, R.NV12) == ERR_ARG
    drv.close()
    host_params = api.NativeDriver(W, H, device_params=0)
    assert lib.vp8drv_set_source_format(host_params.h, R.NV12) == ERR_ARG
    with pytest.raises(api.Vp8HipError) as e:
        host_params.set_source_format("nv12")
    assert e.value.args[1] == ERR_ARG
    host_params.close()


# ---- 7. the tools -------------------------------------------------------------------------------------------------------------------------
def test_the_tools_take_the_format_from_the_c_tag(tmp_path, sequence):
    import os
    import shutil
    import subprocess
    import sys
    from vp8oclenc_amd import y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exes = {}
    for name in ("y4m_to_ivf", "y4m_to_ivf_gops"):
        exes[name] = str(tmp_path / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(root, "include"), os.path.join(root, "scripts", "native", name + ".cpp"), "-o", exes[name],
                        "-L", os.path.join(root, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(root, "vp8oclenc_amd")], check=True, timeout=300)
    # 4:2:2 and 10-bit 4:2:0 files whose frames are NOT a replicated I420 frame: random chroma, junk in the unused bits
    files = {}
    for tag, fmt in (("C422", R.I422), ("C420p10", R.I010)):
        frames = [R.make_planes(fmt, *R.random_samples(fmt, W, H, 300 + t), junk=np.full((H, W), 21)) for t in range(3)]
        y4m.write_y4m(str(tmp_path / f"{tag}.y4m"), frames, framerate=25, tag=tag, size=(W, H))
        y4m.write_y4m(str(tmp_path / f"{tag}_as_i420.y4m"), [R.convert_ref(fmt, W, H, f) for f in frames], framerate=25)
        files[tag] = frames
    y4m.write_y4m(str(tmp_path / "mono.y4m"), [[np.zeros(W * H, np.uint8)]], tag="Cmono", size=(W, H))

    def run(exe, src, out, *extra, ok=True):
        r = subprocess.run([exes[exe], str(tmp_path / src), str(tmp_path / out), "-g", "3"] + list(extra), capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read() if ok else r.stderr
    for tag in files:
        assert run("y4m_to_ivf", f"{tag}.y4m", f"{tag}.ivf") == run("y4m_to_ivf", f"{tag}_as_i420.y4m", f"{tag}_direct.ivf"), tag
        assert "colourspace" in run("y4m_to_ivf_gops", f"{tag}.y4m", "no.ivf", ok=False)
    assert "Cmono" in run("y4m_to_ivf", "mono.y4m", "no.ivf", ok=False)
    # -input-format: frames the header cannot describe (NV12 under a C420 tag)
    nv = [R.make_planes(R.NV12, *R.random_samples(R.NV12, W, H, 400 + t)) for t in range(3)]
    y4m.write_y4m(str(tmp_path / "nv12.y4m"), nv, framerate=25, tag="C420", size=(W, H))
    y4m.write_y4m(str(tmp_path / "nv12_as_i420.y4m"), [R.convert_ref(R.NV12, W, H, f) for f in nv], framerate=25)
    assert run("y4m_to_ivf", "nv12.y4m", "nv12.ivf", "-input-format", "nv12") == run("y4m_to_ivf", "nv12_as_i420.y4m", "nv12_direct.ivf")
    assert "-input-format" in run("y4m_to_ivf", "nv12.y4m", "no.ivf", "-input-format", "yuy2", ok=False)

    # the Python tool
    def py(src, out, *extra, ok=True):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "encode_ivf.py"), str(tmp_path / out), "--y4m", str(tmp_path / src), "--gop", "3"] + list(extra),
                           capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read() if ok else r.stderr
    assert py("C420p10.y4m", "py10.ivf") == py("C420p10_as_i420.y4m", "py10_direct.ivf")
    assert py("nv12.y4m", "pynv.ivf", "--source-format", "nv12") == py("nv12_as_i420.y4m", "pynv_direct.ivf")
    assert "Cmono" in py("mono.y4m", "no.ivf", ok=False)
    f = y4m.Y4mFile(str(tmp_path / "C422.y4m"))
    assert (f.format, f.n) == (R.I422, 3) and all(np.array_equal(a, b) for a, b in zip(f.planes(1), files["C422"][1]))
    with pytest.raises(ValueError):
        f.frame(0)
