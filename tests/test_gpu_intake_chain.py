"""Every way a frame becomes current runs the same chain -- convert, deinterlace, scale (or pack), denoise, analysis -- in the same order:
one configuration with every stage on, the same frames through the six ways in (a context fed from device memory, from host memory,
from host memory prefetched; a batch of two fed from device memory, from host memory, from host memory prefetched), each on fresh
contexts.  The surfaces and the three records of every frame are those of the first way, and the first way's are the numpy chain's:
packed_format_ref.convert_ref -> deinterlace_ref.Deinterlacer -> the scale restatement of test_scale_cpu.py -> denoise_ref.Denoiser ->
analysis_ref.source_side.  Everything is exact: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import analysis_ref
import deinterlace_ref
import denoise_ref
import packed_format_ref as P
from test_gpu_deinterlace import assert_surfaces, current_surfaces
from test_scale_cpu import AREA, lib_taps, pad_plane, ref_scale_frame

pytestmark = pytest.mark.gpu

# BGRA frames of 112x80, read with BT.709 limited range, deinterlaced (adaptive, bottom field kept), scaled to 56x40 (area filter) in a
# coded frame of 64x48 (padding on both sides, a partial last strip, chroma 28 wide), denoised at level 2, analysed
CODED, IN, DST = (64, 48), (112, 80), (56, 40)
MATRIX, DI_MODE, DI_KEEP, DN_LEVEL, FRAMES = P.BT709_LIMITED, 2, 1, 2, 5
SEEDS = (41, 42)      # a batch's second member takes in another video
WAYS = ["device", "upload", "prefetch", "batch device", "batch upload", "batch prefetch"]


def make_context():
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(*CODED)
    hip.set_analysis(True)      # (the setters in another order than the stages)
    hip.set_denoise(DN_LEVEL)
    hip.set_source_scaling(IN[0], IN[1], DST[0], DST[1], AREA)
    hip.set_deinterlace(DI_MODE, DI_KEEP)
    hip.set_source_colour(MATRIX)
    hip.set_source_format(P.BGRA)
    return hip


def videos():
    return [[P.rgb_near_i420(P.BGRA, *f) for f in deinterlace_ref.interlaced_video(IN[0], IN[1], FRAMES, seed=s, keep=DI_KEEP)] for s in SEEDS]


def observe(hip):
    """what a frame left behind: the current surfaces, the deinterlacer's and the denoiser's records, the analysis record's source side"""
    di, dn, an = hip.deinterlace_result(), hip.denoise_result(), hip.analysis_result()
    return {"surfaces": current_surfaces(hip), "deinterlace": (di.frame_number, di.woven, di.missing),
            "denoise": (dn.frame_number, dn.mbs_filtered, dn.mbs_total),
            "analysis": (an.frame_number, an.coded) + tuple(int(getattr(an, k)) for k in analysis_ref.SOURCE_FIELDS)}


def three(ptr):
    return [ptr, ptr, ptr]      # (one plane: the second and third pointers are never read)


def run_alone(way, video):
    from vp8oclenc_amd import api
    hip = make_context()
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    host = [api.HostBuffer(f) for f in video] if way == "prefetch" else []
    out = []
    for t, f in enumerate(video):
        if way == "device":
            d = api.to_device(f)
            hip.set_current_device(*three(d.data_ptr()))
            hip.synchronize()
            d.free()
        elif way == "upload":
            hip.upload_current(f, f, f)
        else:      # frame t was started on its way behind frame t - 1
            if t == 0:
                assert lib.vp8hip_prefetch_current(hip.h, *three(host[0].data_ptr())) == 0
            assert lib.vp8hip_upload_current(hip.h, *three(host[t].data_ptr())) == 0
            if t + 1 < len(video):
                assert lib.vp8hip_prefetch_current(hip.h, *three(host[t + 1].data_ptr())) == 0
        out.append(observe(hip))
    hip.close()
    for hb in host:
        hb.free()
    return out


def run_batch(way, vids):
    from vp8oclenc_amd import api
    n = len(vids)
    members = [make_context() for _ in range(n)]
    lib = members[0].lib
    arr = C.POINTER(C.c_void_p)
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), arr, C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    lib.vp8hip_batch_set_current_device.argtypes = [C.c_void_p, C.POINTER(C.c_int), arr, arr, arr]
    lib.vp8hip_batch_upload_current.argtypes = [C.c_void_p, C.POINTER(C.c_int), arr, arr, arr]
    lib.vp8hip_batch_prefetch_current.argtypes = [C.c_void_p, arr, arr, arr]
    hb = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * n)(*[m.h for m in members]), n) == 0
    device = way == "batch device"
    bufs = [[(api.to_device if device else api.HostBuffer)(f) for f in v] for v in vids]      # (they stay until the batch has gone)
    planes = lambda t: three((C.c_void_p * n)(*[bufs[i][t].data_ptr() for i in range(n)]))
    out = [[] for _ in range(n)]
    for t in range(FRAMES):
        if device:
            assert lib.vp8hip_batch_set_current_device(hb, None, *planes(t)) == 0
        else:
            if way == "batch prefetch" and t == 0:
                assert lib.vp8hip_batch_prefetch_current(hb, *planes(0)) == 0
            assert lib.vp8hip_batch_upload_current(hb, None, *planes(t)) == 0
            if way == "batch prefetch" and t + 1 < FRAMES:
                assert lib.vp8hip_batch_prefetch_current(hb, *planes(t + 1)) == 0
        for i, m in enumerate(members):
            m.synchronize()
            out[i].append(observe(m))
    lib.vp8hip_batch_destroy(hb)
    for m in members:
        m.close()
    for v in bufs:
        for b in v:
            b.free()
    return out


@pytest.fixture(scope="module")
def first_way():
    """both videos through vp8hip_set_current_device, each on a context of its own: what every other way is held to (computed once)"""
    vids = videos()
    return vids, [run_alone("device", v) for v in vids]


def test_the_first_way_is_the_numpy_chain(first_way):
    vids, got = first_way
    for video, frames in zip(vids, got):
        di, dn = deinterlace_ref.Deinterlacer(DI_MODE, DI_KEEP), denoise_ref.Denoiser(DN_LEVEL)
        prev, woven, filtered = None, 0, 0
        for t, (f, g) in enumerate(zip(video, frames)):
            progressive, n, missing = di.take(P.convert_ref(P.BGRA, IN[0], IN[1], f, MATRIX))
            y, u, v = ref_scale_frame(*progressive, DST[0], DST[1], AREA, lib_taps)
            scaled = (pad_plane(y, *CODED), pad_plane(u, CODED[0] // 2, CODED[1] // 2), pad_plane(v, CODED[0] // 2, CODED[1] // 2))
            clean, m, _ = dn.take(scaled)
            assert_surfaces(g["surfaces"], clean, f"frame {t}")
            assert g["deinterlace"] == (t, n, missing) and missing == IN[0] * IN[1] // 2, t
            assert g["denoise"][:2] == (t, m), t
            want = analysis_ref.source_side(clean[0], prev)
            assert g["analysis"] == (t, 0) + tuple(want[k] for k in analysis_ref.SOURCE_FIELDS), t
            prev = clean[0]
            woven += n
            filtered += m
        assert woven > 0 and filtered > 0      # (the stages did something)


@pytest.mark.parametrize("way", WAYS[1:])
def test_every_way_in_leaves_what_the_first_way_leaves(first_way, way):
    vids, want = first_way
    got = run_batch(way, vids) if way.startswith("batch") else [run_alone(way, vids[0])]
    for i, frames in enumerate(got):
        assert len(frames) == FRAMES
        for t, (g, w) in enumerate(zip(frames, want[i])):
            assert_surfaces(g["surfaces"], w["surfaces"], f"{way}: member {i} frame {t}")
            for k in ("deinterlace", "denoise", "analysis"):
                assert g[k] == w[k], (way, i, t, k, g[k], w[k])
        assert sum(g["deinterlace"][1] for g in frames) > 0 and sum(g["denoise"][1] for g in frames) > 0, (way, i)
