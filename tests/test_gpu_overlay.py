"""Overlays on the device (vp8hip_set_overlay_host / _device, k_overlay_prepare, k_overlay_b) through the C ABI: the kernels against
the rule in plain C++ (vp8host_overlay_frame, which tests/test_overlay_cpu.py holds to the numpy restatement tests/overlay_ref.py) byte
for byte, the padding samples included; several layers, clearing and moving; every route a frame becomes current by; a batch whose
members have different layers or none; the compositions with the scaler, the tone mapper, the orientation and the denoiser; the
bit-exact consequence at driver level -- a driver with a layer codes the bytes of a plain driver fed the composed frames, with and
without scene detection; one 1920x1080 frame; and the setters' refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import denoise_ref
import overlay_ref as R
from test_overlay_cpu import ALPHAS, LAYERS, OPACITIES, layer, picture, positions

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


def coded_size(w, h):
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


def context(pw, ph, coded=None):
    from vp8oclenc_amd import api
    coded = coded or coded_size(pw, ph)
    hip = api.Vp8Hip(*coded)
    if coded != (pw, ph):
        hip.set_source_size(pw, ph)
    return hip, coded


def take_device(hip, dev):
    """dev: the frame's planes in device memory"""
    hip.set_current_device(*[b.data_ptr() for b in dev])
    hip.synchronize()
    return current_surfaces(hip)


def composed(layers, frame, coded):
    """pad(overlay_frame(picture)) with the host function, the layers in slot order"""
    from vp8oclenc_amd import api
    for px, x, y, opacity, fmt, matrix in layers:
        frame = api.overlay_frame(px, x, y, opacity, frame, fmt, matrix)
    return R.pad(frame, *coded)


# ---- 1. the kernels against the rule ------------------------------------------------------------------------------------------------
# padding in both directions; none; a picture narrower than a lane's unit; several workgroups and a ragged edge
@pytest.mark.parametrize("pic,coded", [((40, 26), (48, 32)), ((48, 32), (48, 32)), ((2, 2), (16, 16)), ((130, 66), (144, 80))])
def test_kernel_equals_the_rule_byte_for_byte(pic, coded):
    from vp8oclenc_amd import api
    pw, ph = pic
    hip, coded = context(pw, ph, coded)
    src = picture(pw, ph, seed=11)
    dev = [api.to_device(p) for p in src]
    cases = []
    n = 0
    for (lw, lh), (x, y) in itertools.product(LAYERS, positions(pw, ph)):
        for k, alpha in enumerate(ALPHAS):      # (every alpha kind and, in turn, every opacity, matrix and format at every layer and position)
            cases.append((lw, lh, x, y, alpha, OPACITIES[(n + k) % 5], (n + k) % 4, (R.BGRA, R.RGBA)[(n >> 1) & 1]))
        n += 1
    cases += [(37, 21, 3, 2, alpha, opacity, 1, R.BGRA) for alpha, opacity in itertools.product(ALPHAS, OPACITIES)]
    for n, (lw, lh, x, y, alpha, opacity, matrix, fmt) in enumerate(cases):
        px = layer(lw, lh, alpha, seed=n)
        if n & 1:      # from device memory, rows 12 bytes further apart than the layer is wide
            wide = np.full((lh, lw + 3, 4), 0xa5, np.uint8)
            wide[:, :lw] = px
            d = api.to_device(wide)
            hip.set_overlay(0, d, x, y, opacity, fmt, matrix, lw=lw, lh=lh, pitch=4 * (lw + 3))
        else:
            d = None
            hip.set_overlay(0, px, x, y, opacity, fmt, matrix)
        got = take_device(hip, dev)
        if d:
            d.free()
        assert_surfaces(got, composed([(px, x, y, opacity, fmt, matrix)], src, coded), f"picture {pic} layer {lw}x{lh} at ({x}, {y}) alpha {alpha} opacity {opacity} matrix {matrix} format {fmt}")
    hip.clear_overlay(-1)
    assert_surfaces(take_device(hip, dev), R.pad(src, *coded), "after clear_overlay(-1): the frame as it came")
    hip.close()
    for b in dev:
        b.free()


# ---- 2. several layers, clearing, moving ------------------------------------------------------------------------------------------------
def test_four_overlapping_layers_clear_and_placement():
    from vp8oclenc_amd import api
    pw, ph = 40, 26
    hip, coded = context(pw, ph)
    src = picture(pw, ph, seed=12)
    dev = [api.to_device(p) for p in src]
    layers = [(layer(37, 21, "ramp", 1), -3, -2, 255, R.BGRA, 0), (layer(16, 16, "random", 2), 3, 2, 128, R.RGBA, 1),
              (layer(16, 16, "opaque", 3), 10, 9, 254, R.BGRA, 2), (layer(64, 40, "random", 4), 1, 1, 200, R.RGBA, 3)]
    for k in (2, 0, 3, 1):      # (set in another order than the slots')
        px, x, y, opacity, fmt, matrix = layers[k]
        hip.set_overlay(k, px, x, y, opacity, fmt, matrix)
    assert_surfaces(take_device(hip, dev), composed(layers, src, coded), "four layers in slot order")
    assert not all(np.array_equal(a, b) for a, b in zip(composed(layers, src, coded), composed(layers[::-1], src, coded)))
    hip.clear_overlay(1)
    assert_surfaces(take_device(hip, dev), composed([layers[0]] + layers[2:], src, coded), "slot 1 cleared")
    # a move that changes the parity of x and y and the 4-sample margin, and a fade: equal to setting the layer afresh
    for x, y, opacity in ((11, 10, 254), (12, 9, 77), (-7, 13, 0), (39, 25, 255)):
        hip.set_overlay_placement(2, x, y, opacity)
        moved = [layers[0], layers[2][:1] + (x, y, opacity) + layers[2][4:], layers[3]]
        got = take_device(hip, dev)
        assert_surfaces(got, composed(moved, src, coded), f"slot 2 moved to ({x}, {y}) at opacity {opacity}")
        fresh, _ = context(pw, ph)
        for k, (px, lx, ly, o, fmt, matrix) in zip((0, 2, 3), moved):
            fresh.set_overlay(k, px, lx, ly, o, fmt, matrix)
        assert_surfaces(take_device(fresh, dev), got, "... and a context whose layers were set afresh")
        fresh.close()
    hip.close()
    for b in dev:
        b.free()


# ---- 3. every route gives the same bytes --------------------------------------------------------------------------------------------------
def batch_of(members):
    lib = members[0].lib
    arr = C.POINTER(C.c_void_p)
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), arr, C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    lib.vp8hip_batch_set_current_device.argtypes = [C.c_void_p, C.POINTER(C.c_int), arr, arr, arr]
    lib.vp8hip_batch_upload_current.argtypes = [C.c_void_p, C.POINTER(C.c_int), arr, arr, arr]
    lib.vp8hip_batch_prefetch_current.argtypes = [C.c_void_p, arr, arr, arr]
    hb = C.c_void_p()
    n = len(members)
    assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * n)(*[m.h for m in members]), n) == 0
    return hb


def test_every_route_gives_the_same_bytes():
    from vp8oclenc_amd import api
    pw, ph = 34, 18
    frames = [picture(pw, ph, seed=s) for s in (21, 22, 23)]
    layers = [(layer(16, 16, "ramp", 5), 25, 7, 230, R.BGRA, 1), (layer(5, 3, "random", 6), 1, 1, 255, R.RGBA, 0)]
    coded = coded_size(pw, ph)
    want = [composed(layers, f, coded) for f in frames]

    def make():
        hip, _ = context(pw, ph)
        for k, (px, x, y, o, fmt, matrix) in enumerate(layers):
            hip.set_overlay(k, px, x, y, o, fmt, matrix)
        return hip

    hip = make()
    lib = hip.lib
    lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
    lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
    dev = [[api.to_device(p) for p in f] for f in frames]
    assert_surfaces(take_device(hip, dev[0]), want[0], "set_current_device")
    hip.upload_current(*frames[1])
    assert_surfaces(current_surfaces(hip), want[1], "upload_current")
    host = [[api.HostBuffer(p) for p in f] for f in frames]
    ptrs = [b.data_ptr() for b in host[2]]
    assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
    assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
    assert_surfaces(current_surfaces(hip), want[2], "prefetch_current, then upload_current")
    # a prefetched frame is composed when it is made current, with the layers in force THEN
    assert lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
    hip.set_overlay_placement(0, 2, 3, 100)
    assert lib.vp8hip_upload_current(hip.h, *ptrs) == 0
    moved = [layers[0][:1] + (2, 3, 100) + layers[0][4:], layers[1]]
    assert_surfaces(current_surfaces(hip), composed(moved, frames[2], coded), "a layer moved between prefetch and upload")
    hip.close()
    for way in ("batch device", "batch upload", "batch prefetch"):
        members = [make() for _ in frames]
        hb = batch_of(members)
        bufs = dev if way == "batch device" else host
        plane = lambda k: (C.c_void_p * 3)(*[b[k].data_ptr() for b in bufs])
        if way == "batch device":
            assert lib.vp8hip_batch_set_current_device(hb, None, plane(0), plane(1), plane(2)) == 0
        else:
            if way == "batch prefetch":
                assert lib.vp8hip_batch_prefetch_current(hb, plane(0), plane(1), plane(2)) == 0
            assert lib.vp8hip_batch_upload_current(hb, None, plane(0), plane(1), plane(2)) == 0
        for i, m in enumerate(members):
            m.synchronize()
            assert_surfaces(current_surfaces(m), want[i], f"{way}: member {i}")
        lib.vp8hip_batch_destroy(hb)
        for m in members:
            m.close()
    for f in dev + host:
        for b in f:
            b.free()


# ---- 4. a batch whose members have different layers, or none --------------------------------------------------------------------------------
def test_a_batch_of_three_with_different_layers_and_none():
    from vp8oclenc_amd import api
    pw, ph = 40, 26
    coded = coded_size(pw, ph)
    frames = [picture(pw, ph, seed=s) for s in (31, 32, 33)]
    per_member = [[(layer(5, 3, "random", 7), 35, 23, 255, R.BGRA, 0)],                                              # small, in the corner: its box is its own
                  [],                                                                                                   # no layer: the frame as it came
                  [(layer(64, 40, "ramp", 8), -3, -2, 180, R.RGBA, 3), (layer(16, 16, "opaque", 9), 1, 1, 255, R.BGRA, 2)]]
    members = [context(pw, ph)[0] for _ in frames]
    for m, ls in zip(members, per_member):
        for k, (px, x, y, o, fmt, matrix) in enumerate(ls):
            m.set_overlay(k, px, x, y, o, fmt, matrix)
    hb = batch_of(members)
    lib = members[0].lib
    dev = [[api.to_device(p) for p in f] for f in frames]
    plane = lambda k: (C.c_void_p * 3)(*[b[k].data_ptr() for b in dev])
    assert lib.vp8hip_batch_set_current_device(hb, None, plane(0), plane(1), plane(2)) == 0
    for i, m in enumerate(members):
        m.synchronize()
        assert_surfaces(current_surfaces(m), composed(per_member[i], frames[i], coded), f"member {i}")
    # a subtitle that changes between two frames of the live batch, and one that appears on the member that had none
    per_member[0] = [(layer(37, 21, "random", 10), 2, 4, 255, R.BGRA, 1)]
    per_member[1] = [(layer(16, 16, "ramp", 11), 24, 10, 255, R.RGBA, 0)]
    members[0].set_overlay(0, *per_member[0][0][:4], per_member[0][0][4], per_member[0][0][5])
    members[1].set_overlay(0, *per_member[1][0][:4], per_member[1][0][4], per_member[1][0][5])
    assert lib.vp8hip_batch_set_current_device(hb, None, plane(0), plane(1), plane(2)) == 0
    for i, m in enumerate(members):
        m.synchronize()
        assert_surfaces(current_surfaces(m), composed(per_member[i], frames[i], coded), f"member {i}, second frame")
    lib.vp8hip_batch_destroy(hb)
    for m in members:
        m.close()
    for f in dev:
        for b in f:
            b.free()


# ---- 5. compositions --------------------------------------------------------------------------------------------------------------------------
LOGO = (37, 21, "ramp", 12)


def test_scaler_on_the_layer_is_in_picture_coordinates():
    from vp8oclenc_amd import api
    from test_scale_cpu import AREA, lib_taps, ref_scale_frame
    src, dst, coded = (64, 48), (40, 26), (48, 32)
    hip = api.Vp8Hip(*coded)
    hip.set_source_scaling(src[0], src[1], dst[0], dst[1], AREA)
    px = layer(*LOGO)
    hip.set_overlay(0, px, 9, 7, 240, R.BGRA, 1)
    frame = picture(*src, seed=41)
    dev = [api.to_device(p) for p in frame]
    scaled = ref_scale_frame(*frame, dst[0], dst[1], AREA, lib_taps)
    assert_surfaces(take_device(hip, dev), composed([(px, 9, 7, 240, R.BGRA, 1)], scaled, coded), "64x48 scaled to 40x26, then the layer")
    hip.close()
    for b in dev:
        b.free()


def test_p010_with_a_transfer_then_the_layer():
    from vp8oclenc_amd import api
    import tonemap_ref as T
    pw, ph = 40, 26
    hip, coded = context(pw, ph)
    hip.set_source_format(T.P010)
    hip.set_source_transfer(T.PQ, 1000)
    px = layer(*LOGO)
    hip.set_overlay(0, px, 1, 3, 255, R.RGBA, 0)
    planes = T.make_planes(T.P010, *T.inputs(pw, ph)[0][1:])
    dev = [api.to_device(p) for p in planes]
    hip.set_current_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[1].data_ptr())
    hip.synchronize()
    mapped = api.tonemap_frame(T.P010, T.PQ, 1000, pw, ph, planes, 0)
    assert_surfaces(current_surfaces(hip), composed([(px, 1, 3, 255, R.RGBA, 0)], mapped, coded), "P010 PQ tone-mapped, then the layer")
    hip.close()
    for b in dev:
        b.free()


def test_an_odd_turn_then_the_layer_on_the_upright_picture():
    from vp8oclenc_amd import api
    pw, ph = 40, 26
    hip, coded = context(pw, ph)
    hip.set_source_orientation(1, 0)
    px = layer(*LOGO)
    hip.set_overlay(0, px, 3, 2, 200, R.BGRA, 2)
    raw = picture(ph, pw, seed=43)      # stored sideways: 26 wide, 40 high
    dev = [api.to_device(p) for p in raw]
    upright = api.orient_frame(1, 0, raw)
    assert upright[0].shape == (ph, pw)
    assert_surfaces(take_device(hip, dev), composed([(px, 3, 2, 200, R.BGRA, 2)], upright, coded), "a quarter turn, then the layer")
    hip.close()
    for b in dev:
        b.free()


def test_compose_then_denoise_against_the_previous_composed_and_denoised_frame():
    from vp8oclenc_amd import api
    pw, ph = 40, 26
    hip, coded = context(pw, ph)
    hip.set_denoise(2)
    px = layer(*LOGO)
    lay = (px, 3, 2, 255, R.BGRA, 0)
    hip.set_overlay(0, *lay[:4], lay[4], lay[5])
    video = denoise_ref.sequences(pw, ph, seed=5, frames=3)["static_noise"]      # (of the PICTURE's size: the pack pads them)
    dn = denoise_ref.Denoiser(2)
    filtered = 0
    for t, f in enumerate(video[:3]):
        f = [np.ascontiguousarray(p) for p in f]
        dev = [api.to_device(p) for p in f]
        got = take_device(hip, dev)
        want, n, _ = dn.take(composed([lay], f, coded))
        assert_surfaces(got, want, f"frame {t}: composed, then denoised")
        assert hip.denoise_result().mbs_filtered == n
        filtered += n
        for b in dev:
            b.free()
    assert filtered > 0      # (the denoiser did something, on frames that carry the layer)
    hip.close()


# ---- 6. driver level ----------------------------------------------------------------------------------------------------------------------------
W, H, FRAMES, GOP = 48, 32, 6, 4


@pytest.fixture(scope="module")
def video():
    """six frames with a cut at frame 3 (another seed, U shifted) and still chroma between: the scan's differences are not all alike"""
    from vp8oclenc_amd.synth import SynthSequence
    seqs = [SynthSequence(W, H, seed=61), SynthSequence(W, H, seed=68)]
    out = []
    for t in range(FRAMES):
        k = int(t >= 3)
        y, (_, u, v) = seqs[k].frame(t)[0], seqs[k].frame(0)
        u = np.clip(u.astype(int) + 45 * k, 0, 255).astype(np.uint8)
        out.append(tuple(np.ascontiguousarray(p[:H >> (i > 0), :W >> (i > 0)]) for i, p in enumerate((y, u, v))))
    return out


DRIVER_LAYERS = [(layer(16, 16, "ramp", 13), 29, 3, 255, R.BGRA, 0), (layer(37, 21, "random", 14), -3, 20, 160, R.RGBA, 1)]


def drive(frames, layers=(), clear_at=None, **cfg):
    from vp8oclenc_amd import api
    drv = api.NativeDriver(W, H, gop_size=GOP, check_ssim=1, device_params=1, **cfg)
    for k, (px, x, y, o, fmt, matrix) in enumerate(layers):
        drv.set_overlay(k, px, x, y, o, fmt, matrix)
    out = []
    for t, f in enumerate(frames):
        if t == clear_at:
            drv.clear_overlay(-1)
        drv.encode_frame_host(*f)
        out.append(drv.get_frame())
    scenes = drv.stats().scene_changes
    drv.close()
    return out, scenes


@pytest.mark.parametrize("scene_detect", [0, 1])
def test_a_driver_with_layers_codes_the_bytes_of_a_plain_driver_fed_the_composed_frames(video, scene_detect):
    from vp8oclenc_amd import api
    burnt = [R.overlay_layers(DRIVER_LAYERS, f) for f in video]
    for f, g in zip(video, burnt):      # (the host function makes the same frames)
        for a, b in zip(composed(DRIVER_LAYERS, f, (W, H)), g):
            assert np.array_equal(a, b)
    want, scenes = drive(burnt, scene_detect=scene_detect)
    kinds = [f[0] & 1 for f in want]
    assert kinds[0] == 0 and 1 in kinds
    got, got_scenes = drive(video, DRIVER_LAYERS, scene_detect=scene_detect)
    assert got == want and got_scenes == scenes
    assert drive(video, scene_detect=scene_detect)[0] != want      # (and without the layers the picture is another one)


def test_after_clearing_at_a_scheduled_key_frame_the_frames_are_a_fresh_drivers(video):
    got, _ = drive(video, DRIVER_LAYERS, clear_at=GOP)
    fresh, _ = drive(video[GOP:])
    assert not got[GOP][0] & 1      # frame 4 is the schedule's key frame
    assert got[GOP:] == fresh


# ---- 7. one large frame -----------------------------------------------------------------------------------------------------------------------
def test_a_full_frame_layer_at_1920x1080():
    from vp8oclenc_amd import api
    pw, ph = 1920, 1080
    hip, coded = context(pw, ph)
    src = picture(pw, ph, seed=71)
    px = np.random.default_rng(72).integers(0, 256, (ph, pw, 4), dtype=np.uint8)
    hip.set_overlay(0, px, -1, -1, 255, R.BGRA, 1)
    dev = [api.to_device(p) for p in src]
    assert_surfaces(take_device(hip, dev), composed([(px, -1, -1, 255, R.BGRA, 1)], src, coded), "1920x1080, a full-frame random layer at (-1, -1)")
    hip.close()
    for b in dev:
        b.free()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def overlay_abi(lib):
    for fn in (lib.vp8hip_set_overlay_host, lib.vp8hip_set_overlay_device, lib.vp8drv_set_overlay_host, lib.vp8drv_set_overlay_device):
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 6
    for fn in (lib.vp8hip_set_overlay_placement, lib.vp8drv_set_overlay_placement):
        fn.argtypes = [C.c_void_p] + [C.c_int] * 4
    for fn in (lib.vp8hip_clear_overlay, lib.vp8drv_clear_overlay):
        fn.argtypes = [C.c_void_p, C.c_int]


def test_the_context_setters_refuse_bad_arguments_and_change_nothing():
    from vp8oclenc_amd import api
    pw, ph = 40, 26
    hip, coded = context(pw, ph)
    lib = hip.lib
    overlay_abi(lib)
    px = layer(5, 3, "random", 15)
    src = picture(pw, ph, seed=81)
    dev = [api.to_device(p) for p in src]
    assert lib.vp8hip_clear_overlay(hip.h, -1) == 0                     # no layer: nothing to do
    assert lib.vp8hip_clear_overlay(hip.h, 0) == ERR_ARG                # an empty slot
    assert lib.vp8hip_set_overlay_placement(hip.h, 0, 0, 0, 255) == ERR_ARG
    hip.set_overlay(1, px, 3, 2, 200)
    want = composed([(px, 3, 2, 200, R.BGRA, 0)], src, coded)
    good = dict(slot=1, format=R.BGRA, matrix=0, pixels=px.ctypes.data, lw=5, lh=3, pitch=20, x=3, y=2, opacity=200)
    bad = [dict(slot=-1), dict(slot=4), dict(format=0), dict(format=16), dict(format=20), dict(matrix=-1), dict(matrix=4), dict(pixels=None), dict(lw=0),
           dict(lh=0), dict(lw=16385, pitch=4 * 16385), dict(lh=16385), dict(pitch=19), dict(x=-16385), dict(x=16385), dict(y=-16385), dict(y=16385),
           dict(opacity=-1), dict(opacity=256)]
    for kw in bad:
        for fn in (lib.vp8hip_set_overlay_host, lib.vp8hip_set_overlay_device):
            assert fn(hip.h, *{**good, **kw}.values()) == ERR_ARG, kw
    assert lib.vp8hip_set_overlay_host(None, *good.values()) == ERR_ARG
    for slot, x, y, o in ((-1, 0, 0, 255), (4, 0, 0, 255), (0, 0, 0, 255), (1, 16385, 0, 255), (1, 0, -16385, 255), (1, 0, 0, 256), (1, 0, 0, -1)):
        assert lib.vp8hip_set_overlay_placement(hip.h, slot, x, y, o) == ERR_ARG, (slot, x, y, o)
    for slot in (-2, 4, 0, 2):
        assert lib.vp8hip_clear_overlay(hip.h, slot) == ERR_ARG, slot
    assert_surfaces(take_device(hip, dev), want, "after every refusal the layer is the one that was set")
    hip.close()
    for b in dev:
        b.free()


def test_a_driver_with_host_parameters_refuses_layers():
    from vp8oclenc_amd import api
    drv = api.NativeDriver(W, H, device_params=0)
    lib = drv.lib
    overlay_abi(lib)
    px = layer(5, 3, "random", 16)
    for fn in (lib.vp8drv_set_overlay_host, lib.vp8drv_set_overlay_device):
        assert fn(drv.h, 0, R.BGRA, 0, px.ctypes.data, 5, 3, 20, 0, 0, 255) == ERR_ARG
    assert lib.vp8drv_set_overlay_placement(drv.h, 0, 0, 0, 255) == ERR_ARG
    assert lib.vp8drv_clear_overlay(drv.h, -1) == ERR_ARG
    drv.close()


def test_a_context_in_a_by_reference_split_refuses_layers():
    from vp8oclenc_amd import api, ref_shard
    be = ref_shard.HipRefBackend(W, H)
    lib = be.lib
    overlay_abi(lib)
    be.upload_current(*picture(W, H, seed=82))
    be.shard_init(ref_shard.shard_unique_id(), 0, 1)
    px = layer(5, 3, "random", 17)
    d = api.to_device(px)
    assert lib.vp8hip_set_overlay_host(be.h, 0, R.BGRA, 0, px.ctypes.data, 5, 3, 20, 0, 0, 255) == ERR_STATE
    assert lib.vp8hip_set_overlay_device(be.h, 0, R.BGRA, 0, d.data_ptr(), 5, 3, 20, 0, 0, 255) == ERR_STATE
    assert lib.vp8hip_clear_overlay(be.h, -1) == ERR_STATE
    be.close()
    d.free()
    # ... and a context with a layer joins no split
    hip = api.Vp8Hip(W, H)
    hip.set_overlay(0, px, 0, 0, 255)
    lib.vp8hip_shard_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    assert lib.vp8hip_shard_init(hip.h, ref_shard.shard_unique_id(), 0, 1) == ERR_STATE
    hip.close()


def test_hidden_alt_ref_frames_are_refused_while_a_layer_is_set():
    from vp8oclenc_amd import api
    import arf_ref as ref
    frames = ref.noisy_pan(W, H, 3, seed=3)
    drv = api.NativeDriver(W, H, device_params=1)
    lib = drv.lib
    for fn in (lib.vp8drv_encode_arf_host, lib.vp8drv_encode_arf_device):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    keep, table = api._plane_table(frames)
    dev = [[api.to_device(p) for p in f] for f in frames]
    dtable = (C.c_void_p * 9)(*[b.data_ptr() for f in dev for b in f])
    drv.set_arf(4)
    drv.encode_frame_host(*frames[0])
    drv.get_frame()
    drv.set_overlay(2, layer(5, 3, "random", 18), 0, 0, 255)
    assert lib.vp8drv_encode_arf_host(drv.h, table, 3, 1) == ERR_ARG
    assert lib.vp8drv_encode_arf_device(drv.h, dtable, 3, 1) == ERR_ARG
    drv.clear_overlay(2)
    assert lib.vp8drv_encode_arf_host(drv.h, table, 3, 1) == 0      # ... and without it the hidden frame is coded
    assert len(drv.get_frame()) > 3
    drv.close()
    for f in dev:
        for b in f:
            b.free()
