"""Pitched, cropped and rotated source frames on the device (vp8hip_set_source_window: k_window_b and the 2-D copies of host planes;
vp8hip_set_source_orientation: k_orient_b): the kernels against the numpy restatement of tests/geometry_ref.py byte for byte whichever
way a frame comes in, composed with every other stage of the input side, through the driver, the refusals, and off.  A context with
the setting, fed surfaces or raw frames, must hold the current surfaces of a plain context fed the restatement's frames.  Everything
is exact: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import analysis_ref
import deinterlace_ref
import denoise_ref
import geometry_ref as ref
from test_gpu_deinterlace import assert_surfaces, current_surfaces
from test_scale_cpu import AREA, lib_taps, pad_plane, ref_scale_frame

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4


class Surface:
    """a surface in one allocation (host, page-locked host or device) that holds `tight` -- the window's planes as (rows, row_bytes)
    byte arrays -- at (x, y) and noise everywhere else; lead: bytes in front of the first plane, so that every base is odd"""

    def __init__(self, fmt, tight, sw, sh, x, y, pitch, seed, where, lead=0):
        from vp8oclenc_amd import api
        rng = np.random.default_rng(seed)
        planes = ref.surface(fmt, sw, sh, pitch, rng)
        for p, (hs, vs, bpe) in enumerate(ref.TABLE[fmt]):
            t = np.ascontiguousarray(tight[p]).view(np.uint8).reshape(tight[p].shape[0], -1)
            planes[p][y >> vs:(y >> vs) + t.shape[0], (x >> hs) * bpe:(x >> hs) * bpe + t.shape[1]] = t
        self.planes = planes
        flat = np.concatenate([rng.integers(0, 256, lead, dtype=np.uint8)] + [p.ravel() for p in planes])
        at = np.cumsum([lead] + [p.size for p in planes])[:len(planes)]
        self.buf = flat if where == "host" else (api.HostBuffer(flat) if where == "pinned" else api.to_device(flat))
        base = flat.ctypes.data if where == "host" else self.buf.data_ptr()
        self.ptrs = [int(base + a) for a in at]
        self.ptrs += [self.ptrs[-1]] * (3 - len(self.ptrs))      # (planes the format lacks: the last one again, never read)

    def free(self):
        if not isinstance(self.buf, np.ndarray):
            self.buf.free()


def take_ptrs(hip, ptrs, way):
    """way device: vp8hip_set_current_device; upload: vp8hip_upload_current; prefetch: vp8hip_prefetch_current, then the upload that finds it"""
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    if way == "device":
        hip.set_current_device(*ptrs)
        hip.synchronize()
        return
    if way == "prefetch":
        assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
    assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0


def take_frame(hip, frame, way):
    from vp8oclenc_amd import api
    if way == "device":
        d = [api.to_device(p) for p in frame]
        hip.set_current_device(*[b.data_ptr() for b in d])
        hip.synchronize()
        for b in d:
            b.free()
    else:
        hip.upload_current(*[np.ascontiguousarray(p) for p in frame])


# ---- 1. the orient kernel ---------------------------------------------------------------------------------------------------------------
# (coded upright size, source size or None, incoming size of a scaler or None).  16x16: chroma 8x8, below any tile; 48x32: not square;
# 50x36: chroma 25 wide, odd, rows at odd bytes; 200x70: several tiles and a tail in one direction, chroma 35 high, odd; 128x96 scaled
# to 64x48: the scaler reads the stage's output
SHAPES = [((16, 16), None, None), ((48, 32), None, None), ((64, 48), (50, 36), None), ((208, 80), (200, 70), None), ((64, 48), None, (128, 96))]


@pytest.mark.parametrize("way", ["device", "upload"])
@pytest.mark.parametrize("coded,src,scaled", SHAPES)
def test_orient_kernel_equals_the_restatement(coded, src, scaled, way):
    from vp8oclenc_amd import api
    W, H = coded
    iw, ih = scaled or src or coded
    plain, turned = api.Vp8Hip(W, H), api.Vp8Hip(W, H)      # `plain` pads / scales the restatement's frames: what the pack is given
    for hip in (plain, turned):
        if scaled:
            hip.set_source_scaling(iw, ih, W, H, AREA)
        elif src:
            hip.set_source_size(*src)
    for turns, mirror in ref.ORIENTATIONS:
        turned.set_source_orientation(turns, mirror)
        rw, rh = (ih, iw) if turns & 1 else (iw, ih)
        raw = ref.raw_frame(rw, rh, seed=10 * turns + mirror)
        want = ref.orient(raw, turns, mirror)
        assert want[0].shape == (ih, iw)
        take_frame(plain, want, way)
        take_frame(turned, raw, way)
        assert_surfaces(current_surfaces(turned), current_surfaces(plain), f"turns {turns} mirror {mirror}")
    plain.close()
    turned.close()


# ---- 2. the window kernel and the windowed copies ---------------------------------------------------------------------------------------
WINDOW, SURFACE = (48, 32), (80, 48)
WINDOW_FORMATS = [ref.I420, ref.NV12, ref.I444, ref.P010, ref.I210, ref.YUY2, ref.BGRA]
EIGHT_BIT = [ref.I420, ref.NV12, ref.I444, ref.YUY2, ref.BGRA]


@pytest.mark.parametrize("way", ["device", "upload", "prefetch"])
@pytest.mark.parametrize("fmt", WINDOW_FORMATS)
def test_window_equals_the_restatement(fmt, way):
    from vp8oclenc_amd import api
    (w, h), (sw, sh) = WINDOW, SURFACE
    plain, win = api.Vp8Hip(w, h), api.Vp8Hip(w, h)
    for hip in (plain, win):
        hip.set_source_format(fmt)
    rng = np.random.default_rng(200 + fmt)
    where = {"device": "device", "upload": "host", "prefetch": "pinned"}[way]
    cases = [(x, y, extra, 0) for x, y in ref.ORIGINS for extra in ref.EXTRA_PITCH]
    if fmt in EIGHT_BIT:
        cases.append((2, 6, 3, 1))      # the base one byte into its allocation, an odd pitch
    for i, (x, y, extra, lead) in enumerate(cases):
        pitch = [p + extra for p in ref.tight_pitch(fmt, sw)]
        tight = [rng.integers(0, 256, (h >> vs, (w >> hs) * bpe), dtype=np.uint8) for hs, vs, bpe in ref.TABLE[fmt]]
        s = Surface(fmt, tight, sw, sh, x, y, pitch, 300 + i, where, lead)
        for a, b in zip(ref.window(fmt, s.planes, w, h, x, y), tight):
            assert np.array_equal(a, b)
        win.set_source_window(pitch + [0] * (3 - len(pitch)), x, y)
        flat = [t.ravel() for t in tight]
        plain.upload_current(*(flat + [flat[-1]] * (3 - len(flat))))
        take_ptrs(win, s.ptrs, way)
        assert_surfaces(current_surfaces(win), current_surfaces(plain), f"format {fmt} at ({x}, {y}) pitch +{extra} lead {lead}")
        win.synchronize()
        s.free()
    plain.close()
    win.close()


# ---- 3. composition: every stage on, every way in ---------------------------------------------------------------------------------------
# an NV12 surface of 96x128 (pitch 99) whose window of 80x112 at (2, 6) is deinterlaced (adaptive, bottom field kept), mirrored and
# turned once into 112x80, scaled to 56x40 in a coded frame of 64x48, denoised at level 2, analysed
CODED, IN, DST, RAW, SURF = (64, 48), (112, 80), (56, 40), (80, 112), (96, 128)
ORIGIN, PITCH, TURNS, MIRROR = (2, 6), [99, 99, 0], 1, 1
DI_MODE, DI_KEEP, DN_LEVEL, FRAMES = 2, 1, 2, 4
SEEDS = (51, 52)
WAYS = ["device", "upload", "prefetch", "batch device", "batch upload", "batch prefetch"]


def make_context():
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(*CODED)
    hip.set_analysis(True)      # (the setters in another order than the stages)
    hip.set_source_orientation(TURNS, MIRROR)
    hip.set_denoise(DN_LEVEL)
    hip.set_source_scaling(IN[0], IN[1], DST[0], DST[1], AREA)
    hip.set_source_format(ref.NV12)
    hip.set_source_window(PITCH, *ORIGIN)
    hip.set_deinterlace(DI_MODE, DI_KEEP)
    return hip


def videos():
    return [deinterlace_ref.interlaced_video(RAW[0], RAW[1], FRAMES, seed=s, keep=DI_KEEP) for s in SEEDS]


def nv12_surfaces(video, where):
    from vp8oclenc_amd import api
    out = []
    for t, f in enumerate(video):
        y, uv = api.planes_from_i420(api.FORMAT_NV12, *f)[:2]
        tight = [y.reshape(RAW[1], RAW[0]), uv.reshape(RAW[1] // 2, RAW[0])]
        out.append(Surface(ref.NV12, tight, SURF[0], SURF[1], ORIGIN[0], ORIGIN[1], PITCH[:2], 400 + t, where))
    return out


def observe(hip):
    di, dn, an = hip.deinterlace_result(), hip.denoise_result(), hip.analysis_result()
    return {"surfaces": current_surfaces(hip), "deinterlace": (di.frame_number, di.woven, di.missing),
            "denoise": (dn.frame_number, dn.mbs_filtered, dn.mbs_total),
            "analysis": (an.frame_number, an.coded) + tuple(int(getattr(an, k)) for k in analysis_ref.SOURCE_FIELDS)}


def run_alone(way, video):
    hip = make_context()
    surfaces = nv12_surfaces(video, {"device": "device", "upload": "host", "prefetch": "pinned"}[way])
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    out = []
    for t, s in enumerate(surfaces):
        if way == "prefetch":      # frame t was started on its way behind frame t - 1
            if t == 0:
                assert lib.vp8hip_prefetch_current(hip.h, *s.ptrs) == 0
            assert lib.vp8hip_upload_current(hip.h, *s.ptrs) == 0
            if t + 1 < len(surfaces):
                assert lib.vp8hip_prefetch_current(hip.h, *surfaces[t + 1].ptrs) == 0
        else:
            take_ptrs(hip, s.ptrs, way)
        out.append(observe(hip))
    hip.close()
    for s in surfaces:
        s.free()
    return out


def run_batch(way, vids):
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
    surfaces = [nv12_surfaces(v, "device" if device else "pinned") for v in vids]      # (they stay until the batch has gone)
    planes = lambda t: [(C.c_void_p * n)(*[surfaces[i][t].ptrs[k] for i in range(n)]) for k in range(3)]
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
    for v in surfaces:
        for s in v:
            s.free()
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
            progressive, n, missing = di.take(f)      # (the window of the surface, converted: the I420 frame the NV12 planes carry)
            upright = ref.orient(progressive, TURNS, MIRROR)
            assert upright[0].shape == (IN[1], IN[0])
            y, u, v = ref_scale_frame(*upright, DST[0], DST[1], AREA, lib_taps)
            scaled = (pad_plane(y, *CODED), pad_plane(u, CODED[0] // 2, CODED[1] // 2), pad_plane(v, CODED[0] // 2, CODED[1] // 2))
            clean, m, _ = dn.take(scaled)
            assert_surfaces(g["surfaces"], clean, f"frame {t}")
            assert g["deinterlace"] == (t, n, missing) and missing == RAW[0] * RAW[1] // 2, t
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
    got = run_batch(way, vids) if way.startswith("batch") else [run_alone(way, vids[0])]      # (the batch equals its two members alone)
    for i, frames in enumerate(got):
        assert len(frames) == FRAMES
        for t, (g, w) in enumerate(zip(frames, want[i])):
            assert_surfaces(g["surfaces"], w["surfaces"], f"{way}: member {i} frame {t}")
            for k in ("deinterlace", "denoise", "analysis"):
                assert g[k] == w[k], (way, i, t, k, g[k], w[k])


# ---- 4. the driver, end to end ----------------------------------------------------------------------------------------------------------
DRV_CFG = dict(gop_size=3, altref_range=2, check_ssim=1, ref_mask=3, num_partitions=2, quality_stats=1, ssim_target=-1.0)
DRV_TURNS, DRV_MIRROR, DRV_ORIGIN, DRV_SURF = 3, 0, (2, 6), (64, 80)


def drv_video(n):
    """n raw frames of 48x64 that drift (the inter frames find motion), upright 64x48 behind three turns"""
    rng = np.random.default_rng(61)
    big = ref.raw_frame(48 + 2 * n, 64 + 2 * n, seed=62)
    out = []
    for t in range(n):
        f = [big[0][2 * t:2 * t + 64, 2 * t:2 * t + 48], big[1][t:t + 32, t:t + 24], big[2][t:t + 32, t:t + 24]]
        out.append([np.clip(p.astype(int) + rng.integers(-2, 3, p.shape), 0, 255).astype(np.uint8) for p in f])
    return out


@pytest.mark.parametrize("way", ["device", "host", "prefetch", "stage"])
def test_a_driver_with_window_and_orientation_equals_a_driver_fed_the_restatements_frames(way):
    from vp8oclenc_amd import api
    W, H, n = 64, 48, 4
    pitch = [p + 3 for p in ref.tight_pitch(ref.I420, DRV_SURF[0])]
    a, b = api.NativeDriver(W, H, **DRV_CFG), api.NativeDriver(W, H, **DRV_CFG)
    a.set_source_orientation(DRV_TURNS, DRV_MIRROR)
    a.set_source_window(pitch, *DRV_ORIGIN)
    raw = drv_video(n)
    surfaces = [Surface(ref.I420, f, DRV_SURF[0], DRV_SURF[1], DRV_ORIGIN[0], DRV_ORIGIN[1], pitch, 500 + t, "device" if way == "device" else "pinned")
                for t, f in enumerate(raw)]
    a.lib.vp8drv_stage_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    kinds = []
    for t, (f, s) in enumerate(zip(raw, surfaces)):
        if way == "device":
            a.encode_frame_device(*s.ptrs)
        elif way == "prefetch":
            if t == 0:
                a.prefetch_frame_host_ptr(*s.ptrs)
            a.encode_frame_host_ptr(*s.ptrs)
            if t + 1 < n:
                a.prefetch_frame_host_ptr(*surfaces[t + 1].ptrs)
        else:      # host; stage: frame t was handed over early behind frame t - 1, below
            a.encode_frame_host_ptr(*s.ptrs)
        b.encode_frame_host(*ref.orient(f, DRV_TURNS, DRV_MIRROR))
        fa, fb = a.get_frame(), b.get_frame()
        assert fa == fb, f"{way}: frame {t}: {len(fa)} vs {len(fb)} bytes"
        assert bytes(a.frame_quality()) == bytes(b.frame_quality()), (way, t)
        for p, q in zip(a.hip.download_last(), b.hip.download_last()):
            assert np.array_equal(p, q), (way, t)
        assert a.resolve() == b.resolve()
        kinds.append(not (fa[0] & 1))
        if way == "stage" and t + 1 < n:
            assert a.lib.vp8drv_stage_frame_host(a.h, *surfaces[t + 1].ptrs) == 0
    assert kinds == [True, False, False, True]      # key plus inter
    a.close()
    b.close()
    for s in surfaces:
        s.free()


# ---- 5. refusals and state --------------------------------------------------------------------------------------------------------------
def _set_window(lib, h, pitch, x, y):
    lib.vp8hip_set_source_window.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int]
    return lib.vp8hip_set_source_window(h, None if pitch is None else (C.c_int32 * 3)(*pitch), x, y)


def test_a_refused_setting_leaves_the_previous_one_in_force():
    from vp8oclenc_amd import api
    w, h = WINDOW
    hip, plain = api.Vp8Hip(w, h), api.Vp8Hip(w, h)
    lib = hip.lib
    lib.vp8hip_set_source_orientation.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8hip_set_source_format.argtypes = [C.c_void_p, C.c_int]
    lib.vp8hip_set_source_scaling.argtypes = [C.c_void_p] + [C.c_int] * 5
    pitch = [83, 43, 43]
    hip.set_source_window(pitch, 2, 6)
    hip.set_source_orientation(2, 1)
    for bad in ((pitch, 1, 6), (pitch, 2, 5), (pitch, -2, 6), (pitch, 2, -2), ([49, 43, 43], 2, 6), ([83, 24, 43], 2, 6), ([83, 43, 24], 2, 6), (pitch, 36, 6)):
        assert _set_window(lib, hip.h, *bad) == ERR_ARG, bad
    for bad in ((4, 0), (-1, 0), (0, 2), (1, -1)):
        assert lib.vp8hip_set_source_orientation(hip.h, *bad) == ERR_ARG, bad
    assert lib.vp8hip_set_source_format(hip.h, ref.BGRA) == ERR_ARG              # rows of 200 bytes in a pitch of 83
    assert lib.vp8hip_set_source_scaling(hip.h, 96, 64, w, h, AREA) == ERR_ARG   # rows of 98 bytes
    assert lib.vp8hip_set_source_orientation(hip.h, 1, 0) == 0                   # 32 wide: the window fits; back
    assert lib.vp8hip_set_source_orientation(hip.h, 2, 1) == 0
    f = ref.raw_frame(w, h, seed=70)
    s = Surface(ref.I420, f, 80, 48, 2, 6, pitch, 71, "host")
    take_ptrs(hip, s.ptrs, "upload")      # coding a frame shows what is in force: the window at (2, 6), turned twice behind a mirror
    plain.upload_current(*ref.orient(f, 2, 1))
    assert_surfaces(current_surfaces(hip), current_surfaces(plain), "after refusals")
    hip.close()
    plain.close()
    tall = api.Vp8Hip(32, 48)             # an orientation that would make the window in force invalid
    tall.set_source_window([34, 17, 17], 2, 0)
    assert lib.vp8hip_set_source_orientation(tall.h, 1, 0) == ERR_ARG               # raw 48 wide: rows of 50 bytes
    assert lib.vp8hip_set_source_orientation(tall.h, 2, 0) == 0
    tall.close()
    thin = api.Vp8Hip(16, 16)             # a raw height below 4 under a deinterlacer
    thin.set_source_size(2, 16)
    thin.set_deinterlace(1, 0)
    assert lib.vp8hip_set_source_orientation(thin.h, 1, 0) == ERR_ARG
    assert lib.vp8hip_set_source_orientation(thin.h, 2, 1) == 0
    thin.close()
    assert _set_window(lib, None, pitch, 0, 0) == ERR_ARG and lib.vp8hip_set_source_orientation(None, 0, 0) == ERR_ARG


@pytest.mark.parametrize("what", ["pitch", "origin", "turns", "mirror", "window on and off"])
def test_members_that_differ_make_no_batch(what):
    from vp8oclenc_amd import api
    W, H = 64, 48
    settings = {"pitch": (([64, 32, 32], 0, 0, 0, 0), ([67, 32, 32], 0, 0, 0, 0)), "origin": (([80, 40, 40], 0, 0, 0, 0), ([80, 40, 40], 2, 0, 0, 0)),
                "turns": ((None, 0, 0, 2, 0), (None, 0, 0, 0, 0)), "mirror": ((None, 0, 0, 2, 0), (None, 0, 0, 2, 1)),
                "window on and off": (([64, 32, 32], 0, 0, 0, 0), (None, 0, 0, 0, 0))}[what]
    drvs = [api.NativeDriver(W, H, gop_size=3), api.NativeDriver(W, H, gop_size=3)]
    ctxs = [api.Vp8Hip(W, H), api.Vp8Hip(W, H)]
    for group in (drvs, ctxs):
        for m, (pitch, x, y, turns, mirror) in zip(group, settings):
            m.set_source_window(pitch, x, y)
            m.set_source_orientation(turns, mirror)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(drvs)
    lib = ctxs[0].lib
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    h = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(h), (C.c_void_p * 2)(ctxs[0].h, ctxs[1].h), 2) == ERR_ARG
    for m in drvs + ctxs:
        m.close()


def test_setters_on_a_member_of_a_live_batch_are_refused():
    from vp8oclenc_amd import api
    drvs = [api.NativeDriver(64, 48, gop_size=3) for _ in range(2)]
    for d in drvs:
        d.set_source_window([67, 35, 35], 2, 2)
        d.set_source_orientation(2, 0)
    batch = api.NativeBatch(drvs)
    lib = drvs[0].lib
    lib.vp8drv_set_source_window.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int]
    lib.vp8drv_set_source_orientation.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert lib.vp8drv_set_source_window(drvs[0].h, None, 0, 0) == ERR_STATE
    assert lib.vp8drv_set_source_window(drvs[1].h, (C.c_int32 * 3)(80, 40, 40), 0, 0) == ERR_STATE
    assert lib.vp8drv_set_source_orientation(drvs[0].h, 0, 0) == ERR_STATE
    batch.close()
    assert lib.vp8drv_set_source_orientation(drvs[0].h, 0, 0) == 0      # the batch has gone
    for d in drvs:
        d.close()
    mirror = api.NativeDriver(64, 48, device_params=0)
    assert lib.vp8drv_set_source_window(mirror.h, (C.c_int32 * 3)(80, 40, 40), 0, 0) == ERR_ARG      # the host mirror would scan the caller's luma
    assert lib.vp8drv_set_source_orientation(mirror.h, 2, 0) == ERR_ARG
    mirror.close()


@pytest.mark.parametrize("setter", ["window", "orientation", "deinterlace", "source size"])
def test_a_pending_prefetch_is_dropped_by_either_setter(setter):
    """one rule for every setter that changes what the raw planes mean: planes staged under the old settings are handed over again"""
    from vp8oclenc_amd import api
    w, h = WINDOW
    hip, plain = api.Vp8Hip(w, h), api.Vp8Hip(w, h)
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    pitch = ref.tight_pitch(ref.I420, 80)
    hip.set_source_window(pitch, 0, 0)
    first = ref.raw_frame(w, h, seed=80)
    if setter == "source size":     # 34x18 inside 48x32 while the planes are staged, 36x18 when they are taken (fewer than 16 below the coded width, both)
        hip.set_source_size(34, 18)
        first, (w, h) = ref.raw_frame(34, 18, seed=80), (36, 18)
        plain.set_source_size(w, h)
    second = ref.raw_frame(w, h, seed=81)
    s = Surface(ref.I420, first, 80, 48, 0, 0, pitch, 82, "pinned")
    assert lib.vp8hip_prefetch_current(hip.h, *s.ptrs) == 0
    if setter == "window":      # the same planes through another window: the bytes staged through the first one are not this frame
        hip.set_source_window(pitch, 14, 2)
        want = ref.window(ref.I420, s.planes, w, h, 14, 2)
    else:                       # the setter has waited for the copy: planes rewritten afterwards are read again, or the stale frame shows
        if setter == "orientation":
            hip.set_source_orientation(2, 0)
            want = ref.orient(second, 2, 0)
        elif setter == "deinterlace":
            hip.set_deinterlace(1, 0)
            want = deinterlace_ref.Deinterlacer(1, 0).take(second)[0]
        else:
            hip.set_source_size(w, h)
            want = second
        t = Surface(ref.I420, second, 80, 48, 0, 0, pitch, 83, "host")
        C.memmove(s.buf.data_ptr(), t.buf.ctypes.data, t.buf.nbytes)
    assert lib.vp8hip_upload_current(hip.h, *s.ptrs) == 0
    plain.upload_current(*want)
    assert_surfaces(current_surfaces(hip), current_surfaces(plain), setter)
    hip.close()
    plain.close()
    s.free()


# ---- 6. off is off ----------------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    from vp8oclenc_amd import api
    frames = drv_video(4)
    upright = [ref.orient(f, 3, 0) for f in frames]
    outs, launches = [], []
    for call in (False, True):
        drv = api.NativeDriver(64, 48, **DRV_CFG)
        if call:      # on, then off again before the first frame and once more between frames
            drv.set_source_window([67, 35, 35], 2, 2)
            drv.set_source_orientation(1, 1)
            drv.set_source_window(None)
            drv.set_source_orientation(0, 0)
        drv.hip.profile_enable(["pack"])
        out = []
        for t, f in enumerate(upright):
            if call and t == 2:
                drv.set_source_orientation(2, 0)
                drv.set_source_orientation(0, 0)
            dev = [api.to_device(p) for p in f]
            drv.encode_frame_device(*[d.data_ptr() for d in dev])
            out.append(drv.get_frame())
            out.append(bytes(drv.frame_quality()))
            for d in dev:
                d.free()
        launches.append(drv.hip.profile_read()["pack"][1])
        drv.close()
        outs.append(out)
    assert outs[0] == outs[1]
    assert launches[0] == launches[1] >= len(frames)      # the launches of the input side: those of a driver that never had the settings
    on = api.NativeDriver(64, 48, **DRV_CFG)
    on.set_source_orientation(3, 0)
    on.set_source_window([48, 24, 24], 0, 0)
    on.hip.profile_enable(["pack"])
    for t, f in enumerate(frames):
        dev = [api.to_device(p) for p in f]
        on.encode_frame_device(*[d.data_ptr() for d in dev])
        assert on.get_frame() == outs[0][2 * t]      # (and on is on: the raw frames through both stages are the upright ones)
        for d in dev:
            d.free()
    assert on.hip.profile_read()["pack"][1] == launches[0] + 2 * len(frames)      # window and orient: one more launch each per frame
    on.close()
