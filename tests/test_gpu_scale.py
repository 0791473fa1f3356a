"""Source frames scaled down to the coded size on the device (vp8hip_set_source_scaling, k_scale_b): the kernel against the numpy
restatement of tests/test_scale_cpu.py bit for bit, against the pyramid's 2:1 filter, and composed with everything downstream of the
surfaces -- a driver that scales is a driver fed the restatement's frames, whichever way the frames come in."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_scale_cpu import AREA, LANCZOS, lib_taps, pad_plane, ref_scale_frame

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PAIRS = [((3840, 2160), (1920, 1080)), ((1920, 1080), (1280, 720)), ((1920, 1080), (640, 360)), ((1280, 720), (1278, 714)), ((130, 98), (66, 34))]


def coded(w, h):
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


def random_frame(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def checkerboards(w, h):
    """an all-0 / all-255 checkerboard and its complement: the Lanczos overshoot must clamp, the intermediate must not wrap"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = (((yy + xx) & 1) * 255).astype(np.uint8)
    b = ((((yy >> 1) + (xx >> 1)) & 1) * 255).astype(np.uint8)
    return (a, np.ascontiguousarray(255 - a[:h // 2, :w // 2]), np.ascontiguousarray(b[:h // 2, :w // 2])), \
           (255 - b, np.ascontiguousarray(a[:h // 2, :w // 2]), np.ascontiguousarray(255 - b[:h // 2, :w // 2]))


def expected_surfaces(frame, dst, kind):
    """the restatement applied to the tables vp8host_scale_taps returns, then copy_with_padding to the coded size"""
    Wc, Hc = coded(*dst)
    y, u, v = ref_scale_frame(*frame, dst[0], dst[1], kind, lib_taps)
    return pad_plane(y, Wc, Hc), pad_plane(u, Wc // 2, Hc // 2), pad_plane(v, Wc // 2, Hc // 2)


def current_surfaces(hip):
    from vp8oclenc_amd import api
    return (hip.debug(api.DBG_PYRAMID, 3, 0), hip.debug(api.DBG_CURRENT_CHROMA, 0), hip.debug(api.DBG_CURRENT_CHROMA, 1))


def assert_surfaces(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


# ---- 4. kernel against restatement, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [AREA, LANCZOS])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_kernel_equals_the_restatement_bit_for_bit(src, dst, kind):
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(*coded(*dst))
    hip.set_source_scaling(src[0], src[1], dst[0], dst[1], kind)
    frames = [random_frame(src[0], src[1], 11 + kind)] + list(checkerboards(*src))
    for i, f in enumerate(frames):
        if i == 1:      # once from device memory: the same launch without the staging copy
            d = [api.to_device(p) for p in f]
            hip.set_current_device(*[b.data_ptr() for b in d])
            hip.synchronize()
        else:
            hip.upload_current(*f)
        assert_surfaces(current_surfaces(hip), expected_surfaces(f, dst, kind), f"{src} -> {dst} kind {kind} frame {i}")
    hip.close()


# ---- 5. cross-check with code that is already trusted -----------------------------------------------------------------------------
def test_area_two_to_one_equals_the_pyramids_first_level():
    from vp8oclenc_amd import api
    from vp8oclenc_amd.synth import SynthSequence
    seq = SynthSequence(3840, 2160, seed=4)
    big = api.NativeDriver(3840, 2160, check_ssim=0)
    for t in range(2):      # the second frame is an inter frame: its pyramid is built
        big.encode_frame_host(*seq.frame(t))
    big.hip.synchronize()
    level1 = big.hip.debug(api.DBG_PYRAMID, 3, 1)
    big.close()
    hip = api.Vp8Hip(1920, 1088)
    hip.set_source_scaling(3840, 2160, 1920, 1080, AREA)
    hip.upload_current(*seq.frame(1))
    luma = hip.debug(api.DBG_PYRAMID, 3, 0)
    hip.close()
    assert level1.shape == (1080, 1920)
    assert np.array_equal(luma[:1080], level1)


# ---- 6. composition ------------------------------------------------------------------------------------------------------------------
def synth_frames(w, h, n, seed):
    from vp8oclenc_amd.synth import SynthSequence
    seq = SynthSequence(w, h, seed=seed)
    return [tuple(np.ascontiguousarray(p[:h >> (i > 0), :w >> (i > 0)]) for i, p in enumerate(seq.frame(t))) for t in range(n)]


def quality_bits(q):
    return bytes(q)


@pytest.mark.parametrize("dst,kind", [((1280, 720), AREA), ((640, 360), LANCZOS)])
def test_a_driver_that_scales_equals_a_driver_fed_the_restatements_frames(dst, kind):
    from vp8oclenc_amd import api
    W, H = 1920, 1080
    Wc, Hc = coded(*dst)
    frames = synth_frames(W, H, 9, seed=21)
    cfg = dict(gop_size=4, altref_range=2, check_ssim=1, num_partitions=2, quality_stats=1, ssim_target=0.9)
    size = dict(src_width=dst[0], src_height=dst[1]) if (Wc, Hc) != dst else {}
    a = api.NativeDriver(Wc, Hc, in_width=W, in_height=H, scale_filter=kind, **size, **cfg)
    b = api.NativeDriver(Wc, Hc, **size, **cfg)
    keys = 0
    for t, f in enumerate(frames):
        small = ref_scale_frame(*f, dst[0], dst[1], kind, lib_taps)
        a.encode_frame_host(*f)
        b.encode_frame_host(*small)
        fa, fb = a.get_frame(), b.get_frame()
        assert fa == fb, f"frame {t}: {len(fa)} vs {len(fb)} bytes"
        keys += not (fa[0] & 1)
        for p, q in zip(a.hip.download_last(), b.hip.download_last()):
            assert np.array_equal(p, q), t
        assert quality_bits(a.frame_quality()) == quality_bits(b.frame_quality()), t
    assert keys >= 3      # at least two whole GOPs
    assert quality_bits(a.quality_summary()) == quality_bits(b.quality_summary())
    a.close()
    b.close()


# ---- 7. every way in gives the same frame --------------------------------------------------------------------------------------------
def _lib_call(drv, name, *ptrs):
    fn = getattr(drv.lib, name)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = fn(drv.h, *ptrs)
    assert rc >= 0, (name, rc)


def test_every_way_in_gives_the_same_frames():
    from vp8oclenc_amd import api
    W, H, dst, kind = 640, 480, (320, 232), LANCZOS
    Wc, Hc = coded(*dst)
    frames = synth_frames(W, H, 6, seed=31)
    cfg = dict(gop_size=4, num_partitions=2, in_width=W, in_height=H, scale_filter=kind, src_width=dst[0], src_height=dst[1])
    ny, nc = W * H, (W // 2) * (H // 2)

    def run(way):
        drv = api.NativeDriver(Wc, Hc, **cfg)
        out = []
        host = [api.HostBuffer(np.concatenate([p.ravel() for p in f])) for f in frames]
        ptrs = [(hb.data_ptr(), hb.data_ptr() + ny, hb.data_ptr() + ny + nc) for hb in host]
        for t, f in enumerate(frames):
            if way == "device":
                d = [api.to_device(p) for p in f]
                drv.encode_frame_device(*[x.data_ptr() for x in d])
            elif way == "host":
                drv.encode_frame_host(*f)
            elif way == "prefetch":
                if t == 0:
                    drv.prefetch_frame_host_ptr(*ptrs[0])
                drv.encode_frame_host_ptr(*ptrs[t])
                if t + 1 < len(frames):
                    drv.prefetch_frame_host_ptr(*ptrs[t + 1])
            else:      # stage: frame t + 1 was prefetched and handed over early behind frame t, below
                drv.encode_frame_host_ptr(*ptrs[t])
            if way == "stage":
                drv.get_frame_begin()
                if t + 1 < len(frames):
                    drv.prefetch_frame_host_ptr(*ptrs[t + 1])
                    _lib_call(drv, "vp8drv_stage_frame_host", *ptrs[t + 1])
                out.append(drv.get_frame_end())
            else:
                out.append(drv.get_frame())
        drv.close()
        for hb in host:
            hb.free()
        return out

    want = run("host")
    small = api.NativeDriver(Wc, Hc, gop_size=4, num_partitions=2, src_width=dst[0], src_height=dst[1])
    for t, f in enumerate(frames):
        small.encode_frame_host(*ref_scale_frame(*f, dst[0], dst[1], kind, lib_taps))
        assert small.get_frame() == want[t], t
    small.close()
    for way in ("device", "prefetch", "stage"):
        got = run(way)
        assert got == want, (way, [i for i, (p, q) in enumerate(zip(got, want)) if p != q])


@pytest.mark.parametrize("host", [False, True])
def test_a_batch_of_four_equals_the_four_alone(host):
    from vp8oclenc_amd import api
    W, H, dst, kind = 640, 480, (400, 300), AREA
    Wc, Hc = coded(*dst)
    n, steps = 4, 5
    seqs = [synth_frames(W, H, steps, seed=40 + i) for i in range(n)]
    cfg = dict(gop_size=3, num_partitions=2, in_width=W, in_height=H, scale_filter=kind, src_width=dst[0], src_height=dst[1])
    alone = []
    for i in range(n):
        drv = api.NativeDriver(Wc, Hc, **cfg)
        out = []
        for f in seqs[i]:
            drv.encode_frame_host(*f)
            out.append(drv.get_frame())
        drv.close()
        alone.append(out)
    drvs = [api.NativeDriver(Wc, Hc, **cfg) for _ in range(n)]
    batch = api.NativeBatch(drvs)
    ny, nc = W * H, (W // 2) * (H // 2)
    for t in range(steps):
        if host:
            bufs = [api.HostBuffer(np.concatenate([p.ravel() for p in s[t]])) for s in seqs]
        else:
            bufs = [api.to_device(np.concatenate([p.ravel() for p in s[t]])) for s in seqs]
        batch.encode_frame_device([(b.data_ptr(), b.data_ptr() + ny, b.data_ptr() + ny + nc) for b in bufs], host=host)
        for i, d in enumerate(drvs):
            assert d.get_frame() == alone[i][t], (t, i)
        for b in bufs:
            b.free()
    batch.close()
    for d in drvs:
        d.close()
    # members that disagree on the scaler do not make a batch
    odd = [api.NativeDriver(Wc, Hc, **cfg), api.NativeDriver(Wc, Hc, **dict(cfg, scale_filter=LANCZOS))]
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(odd)
    for d in odd:
        d.close()


# ---- 8. switching --------------------------------------------------------------------------------------------------------------------
def test_switching_between_frames_gives_what_fresh_contexts_give():
    from vp8oclenc_amd import api
    Wc, Hc = 320, 240
    hip = api.Vp8Hip(Wc, Hc)
    lib = hip.lib
    big, mid, same = random_frame(640, 480, 1), random_frame(480, 360, 2), random_frame(Wc, Hc, 3)
    hip.set_source_scaling(640, 480, 320, 240, AREA)
    hip.upload_current(*big)
    assert_surfaces(current_surfaces(hip), expected_surfaces(big, (320, 240), AREA), "on")
    hip.set_source_scaling(0, 0, 0, 0, 1)
    hip.upload_current(*same)
    assert_surfaces(current_surfaces(hip), same, "off")
    hip.set_source_scaling(480, 360, 316, 236, LANCZOS)
    hip.upload_current(*mid)
    assert_surfaces(current_surfaces(hip), expected_surfaces(mid, (316, 236), LANCZOS), "another size")
    # a prefetch made before a size change is not used: the same three addresses, now planes of another size
    bufs = [api.HostBuffer(np.zeros(640 * 480, np.uint8)) for _ in range(3)]
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp8hip_upload_current.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for b, p in zip(bufs, mid):
        C.memmove(b.data_ptr(), p.ctypes.data, p.size)
    ptrs = [b.data_ptr() for b in bufs]
    assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
    hip.set_source_scaling(640, 480, 320, 240, LANCZOS)
    for b, p in zip(bufs, big):
        C.memmove(b.data_ptr(), p.ctypes.data, p.size)
    assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
    assert_surfaces(current_surfaces(hip), expected_surfaces(big, (320, 240), LANCZOS), "after a stale prefetch")
    # ... and one made at the size in force is
    assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
    assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
    assert_surfaces(current_surfaces(hip), expected_surfaces(big, (320, 240), LANCZOS), "prefetched")
    for b in bufs:
        b.free()
    # refused arguments leave the context as it was
    hip.set_source_scaling(0, 0, 0, 0, 0)
    lib.vp8hip_set_source_scaling.argtypes = [C.c_void_p] + [C.c_int] * 5
    for bad in ((640, 480, 320, 240, 2), (641, 480, 320, 240, 0), (640, 480, 300, 240, 0), (640, 480, 322, 240, 0), (300, 480, 320, 240, 0),
                (1920, 1440, 320, 240, 1), (16386, 480, 320, 240, 0), (640, 480, 320, 0, 0)):
        assert lib.vp8hip_set_source_scaling(hip.h, *bad) == -1, bad      # VP8HIP_ERR_ARG
    hip.upload_current(*same)
    assert_surfaces(current_surfaces(hip), same, "after refusals")
    hip.close()
    with pytest.raises(api.Vp8HipError):
        api.NativeDriver(Wc, Hc, in_width=640, in_height=480, device_params=0)
    with pytest.raises(api.Vp8HipError):
        api.NativeDriver(Wc, Hc, in_width=1920, in_height=1440, scale_filter=LANCZOS)      # 6:1: 36 taps


# ---- 9. the tools ----------------------------------------------------------------------------------------------------------------------
def test_the_tools_resize_option(tmp_path):
    import decode_ivf
    import vp8_decode
    from vp8oclenc_amd import api, y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exes = {}
    for name in ("y4m_to_ivf", "y4m_to_ivf_gops"):
        exes[name] = str(tmp_path / name)
        subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", name + ".cpp"), "-o", exes[name],
                        "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    W, H, dst = 1280, 720, (640, 360)
    frames = synth_frames(W, H, 7, seed=51)
    small = [ref_scale_frame(*f, dst[0], dst[1], AREA, lib_taps) for f in frames]
    y4m.write_y4m(str(tmp_path / "big.y4m"), frames, framerate=25)
    y4m.write_y4m(str(tmp_path / "small.y4m"), small, framerate=25)
    common = ["-g", "3", "-partitions", "2", "-no-scene-detect", "-conformant"]

    def run(exe, src, out, *extra):
        r = subprocess.run([exes[exe], str(tmp_path / src), str(tmp_path / out)] + [c for c in common if exe == "y4m_to_ivf" or c != "-no-scene-detect"] + list(extra),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read()
    resized = run("y4m_to_ivf", "big.y4m", "resized.ivf", "-resize", "640x360")
    direct = run("y4m_to_ivf", "small.y4m", "direct.ivf")
    assert resized == direct
    gops = run("y4m_to_ivf_gops", "big.y4m", "gops.ivf", "-resize", "640x360", "-resize-filter", "area", "-chunks", "2", "-batch", "2")
    assert gops == resized
    assert run("y4m_to_ivf", "big.y4m", "lanczos.ivf", "-resize", "640x360", "-resize-filter", "lanczos") != resized
    Wf, Hf, rate, scale, packets = decode_ivf.read_ivf(str(tmp_path / "resized.ivf"))
    assert (Wf, Hf, rate, len(packets)) == (640, 360, 25, 7)
    drv = api.NativeDriver(640, 368, gop_size=3, num_partitions=2, conformant_stream=1, in_width=W, in_height=H, src_width=640, src_height=360)
    dec = vp8_decode.Decoder()
    for t, (f, pkt) in enumerate(zip(frames, packets)):
        drv.encode_frame_host(*f)
        assert drv.get_frame() == pkt, t
        hdr, planes = dec.decode(pkt)
        assert (hdr.width, hdr.height) == (640, 360) or not hdr.key
        for p, q in zip(planes, drv.hip.download_last()):
            assert np.array_equal(np.asarray(p)[:q.shape[0], :q.shape[1]], q), t
    drv.close()
    # the Python tool
    def py(src, out, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / out), "--y4m", str(tmp_path / src), "--gop", "3",
                            "--partitions", "2"] + list(extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read()
    assert py("big.y4m", "py_resized.ivf", "--resize", "640x360") == py("small.y4m", "py_direct.ivf")
