"""Who refuses whom in the native frame loop, with which code (vp8oclenc_amd/csrc/driver_settings.h): every clause of the driver's
refusal table through the real library.  A driver is brought into a state, is asked for what that state refuses, and answers with the
clause's code; then nothing has moved -- the frame counter stands, and the next three frames are the bytes of a driver in the same state
that was never asked.  What is switched off (hidden alt-refs 0, one layer, period 0, no canvas) is refused only by what refuses it.
And the record of the frame just coded: members of a batch whose key frames are coded in the batched launch, or singly, or who code an
inter frame beside them, report what the same drivers report coded on their own.  64x48; everything is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
W, H = 64, 48
GOOD = dict(gop_size=30, altref_range=31, check_ssim=1, qi_min=10, qi_max=60)      # (scheduled alt-refs off: temporal layers may be asked for)
I422 = 2
TILE = [(W, H, 0, 0, W, H, 0)]
_FRAMES = []


def frames():
    if not _FRAMES:
        from vp8oclenc_amd.synth import SynthSequence
        s = SynthSequence(W, H, seed=11, noise=5)
        _FRAMES.extend(tuple(np.ascontiguousarray(p, np.uint8) for p in s.frame(t)) for t in range(6))
    return _FRAMES


def rc_of(call, *args):
    from vp8oclenc_amd import api
    try:
        call(*args)
    except api.Vp8HipError as e:
        return e.args[1]
    return 0


def batch_rc(drivers):
    """vp8drv_batch_create's code (a batch that comes about is destroyed again)"""
    from vp8oclenc_amd import api
    lib = api.load_library()
    lib.vp8drv_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    lib.vp8drv_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8drv_batch_destroy.restype = None
    h = C.c_void_p()
    rc = lib.vp8drv_batch_create(C.byref(h), (C.c_void_p * len(drivers))(*[d.h for d in drivers]), len(drivers))
    if rc == 0:
        lib.vp8drv_batch_destroy(h)
    return rc


def shard(d):
    """the driver's context joins a by-reference split of one rank (it cannot leave again; its frame calls go on as before)"""
    from vp8oclenc_amd import ref_shard
    d.lib.vp8hip_shard_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    assert d.lib.vp8hip_shard_init(d.hip.h, ref_shard.shard_unique_id(), 0, 1) == 0


def take(d, frame):
    if getattr(d, "_canvas_tiles", 0):
        return d.encode_tiles([frame])
    return d.encode_frame_host(*frame)


def stream(d, n=3, feed=None):
    """the next n frames' bytes (frame t of the sequence is the driver's t-th shown frame)"""
    out = []
    for _ in range(n):
        f = frames()[d.stats().frame_number]
        take(d, feed(f) if feed else f)
        out.append(d.get_frame())
        d.resolve()
    return out


# ---- the asks: (driver, a partner that is fit for a batch) -> the code ------------------------------------------------------------------
def arf_on(d, p):
    return rc_of(d.set_arf, 4)


def arf_off(d, p):
    return rc_of(d.set_arf, 0)


def layers_on(d, p):
    return rc_of(d.set_temporal_layers, 2, 0)


def layers_off(d, p):
    return rc_of(d.set_temporal_layers, 1, 0)


def refresh_on(d, p):
    return rc_of(d.set_intra_refresh, 8)


def refresh_off(d, p):
    return rc_of(d.set_intra_refresh, 0)


def canvas_on(d, p):
    return rc_of(d.set_canvas, TILE)


def canvas_off(d, p):
    return rc_of(d.set_canvas, [])


def membership(d, p):
    """a batch of the driver and the partner, either way round; the partner is nobody's member afterwards"""
    a, b = batch_rc([d, p]), batch_rc([p, d])
    assert a == b and rc_of(p.set_denoise, 0) == 0
    return a


def frame_call(d, p):
    y, u, v = (np.ascontiguousarray(x) for x in frames()[d.stats().frame_number])
    d.lib.vp8drv_encode_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    d.lib.vp8drv_encode_frame_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    a = d.lib.vp8drv_encode_frame_host(d.h, y.ctypes.data, u.ctypes.data, v.ctypes.data, 0)
    b = d.lib.vp8drv_encode_frame_device(d.h, y.ctypes.data, u.ctypes.data, v.ctypes.data, 0)      # (refused before a plane is looked at)
    assert a == b
    return a


def hidden_frame(d, p):
    return rc_of(d.encode_arf_host, frames()[:3], 1)


SETTERS = [("denoise", lambda d, p: rc_of(d.set_denoise, 1)), ("deinterlace", lambda d, p: rc_of(d.set_deinterlace, 1, 0)),
           ("format", lambda d, p: rc_of(d.set_source_format, I422)), ("colour", lambda d, p: rc_of(d.set_source_colour, 1)),
           ("transfer", lambda d, p: rc_of(d.set_source_transfer, 1, 1000)), ("window", lambda d, p: rc_of(d.set_source_window, [W + 16, W // 2 + 8, W // 2 + 8])),
           ("window off", lambda d, p: rc_of(d.set_source_window, None)), ("orientation", lambda d, p: rc_of(d.set_source_orientation, 2, 0)),
           ("analysis", lambda d, p: rc_of(d.set_analysis, True))]


# ---- the states: how a driver gets there (returns how it leaves again, if it has to before it codes on) ----------------------------------
def live_member(d):
    from vp8oclenc_amd import api
    other = api.NativeDriver(W, H, **GOOD)
    batch = api.NativeBatch([d, other])
    return lambda: (batch.close(), other.close())


def layers_in_force_one_asked(d):
    d.set_temporal_layers(2, 0)
    stream(d, 1)
    d.set_temporal_layers(1, 0)


def hidden_frame_shapes_the_references(d):
    d.set_arf(4)
    stream(d, 1)
    d.encode_arf_host(frames()[:3], 1)
    assert len(d.get_frame()) > 3
    d.set_arf(0)


def layers_then_split(d):
    d.set_temporal_layers(2, 0)
    shard(d)
    return lambda: d.set_temporal_layers(1, 0)


def refresh_then_split(d):
    d.set_intra_refresh(8)
    shard(d)
    return lambda: d.set_intra_refresh(0)


def arf_and_a_layer(d):
    d.set_arf(4)
    stream(d, 1)
    d.set_overlay(0, np.full((8, 8, 4), 200, np.uint8), 4, 4)


def arf_and_a_frame(d):
    d.set_arf(4)
    stream(d, 1)


def to_i422(f):
    from vp8oclenc_amd import api
    return api.planes_from_i420(I422, *f)


# name: (configuration on top of GOOD, the way into the state, [(what is asked, the ask, the code)], the frames' form)
STATES = {
    "host parameters": (dict(device_params=0), None, [("arf", arf_on, ERR_ARG), ("arf off", arf_off, 0), ("layers", layers_on, ERR_ARG), ("one layer", layers_off, 0),
                                                       ("refresh", refresh_on, ERR_ARG), ("no refresh", refresh_off, 0), ("canvas", canvas_on, ERR_ARG),
                                                       ("no canvas", canvas_off, ERR_ARG), ("member", membership, ERR_ARG)] + [(n, f, ERR_ARG) for n, f in SETTERS], None),
    "overlapped filter": (dict(overlap_filter=1), None, [("arf", arf_on, ERR_ARG), ("arf off", arf_off, 0), ("layers", layers_on, ERR_ARG), ("member", membership, ERR_ARG)], None),
    "scene detection": (dict(scene_detect=1), None, [("member", membership, ERR_ARG)], None),
    "an SSIM target": (dict(ssim_target=-0.5), None, [("refresh", refresh_on, ERR_ARG), ("no refresh", refresh_off, 0)], None),
    "scheduled alt-refs": (dict(altref_range=5), None, [("layers", layers_on, ERR_ARG), ("one layer", layers_off, 0)], None),
    "a source format": ({}, lambda d: d.set_source_format(I422), [("arf", arf_on, ERR_ARG)], to_i422),
    "a window": ({}, lambda d: d.set_source_window([W, W // 2, W // 2]), [("arf", arf_on, ERR_ARG)], None),
    "a deinterlacer": ({}, lambda d: d.set_deinterlace(1, 0), [("arf", arf_on, ERR_ARG)], None),
    "a denoiser": ({}, lambda d: d.set_denoise(2), [("arf", arf_on, ERR_ARG)], None),
    "analysis": ({}, lambda d: d.set_analysis(True), [("arf", arf_on, ERR_ARG)], None),
    "a member of a live batch": ({}, live_member, [("arf", arf_on, ERR_STATE), ("arf off", arf_off, ERR_STATE), ("layers", layers_on, ERR_STATE), ("one layer", layers_off, 0),
                                                   ("refresh", refresh_on, ERR_STATE), ("no refresh", refresh_off, 0), ("canvas", canvas_on, ERR_STATE),
                                                   ("no canvas", canvas_off, 0)] + [(n, f, ERR_STATE) for n, f in SETTERS], None),
    "a canvas": ({}, lambda d: d.set_canvas(TILE), [("arf", arf_on, ERR_STATE), ("member", membership, ERR_ARG), ("a plain frame", frame_call, ERR_STATE)], None),
    "layers asked for": ({}, lambda d: d.set_temporal_layers(3, 0), [("arf", arf_on, ERR_STATE), ("member", membership, ERR_ARG)], None),
    "layers in force, one asked for": ({}, layers_in_force_one_asked, [("arf", arf_on, ERR_STATE), ("member", membership, ERR_ARG)], None),
    "hidden alt-refs": ({}, lambda d: d.set_arf(4), [("layers", layers_on, ERR_STATE), ("one layer", layers_off, 0), ("canvas", canvas_on, ERR_STATE),
                                                     ("no canvas", canvas_off, 0), ("member", membership, ERR_ARG), ("a hidden frame with no reference", hidden_frame, ERR_STATE)], None),
    "a hidden frame shapes the references": ({}, hidden_frame_shapes_the_references, [("member", membership, ERR_ARG), ("a hidden frame, off", hidden_frame, ERR_STATE)], None),
    "a refresh period": ({}, lambda d: d.set_intra_refresh(8), [("member", membership, ERR_ARG)], None),
    "a by-reference split": ({}, shard, [("layers", layers_on, ERR_STATE), ("one layer", layers_off, 0), ("refresh", refresh_on, ERR_STATE), ("no refresh", refresh_off, 0)], None),
    "layers, then a split": ({}, layers_then_split, [("a frame", frame_call, ERR_STATE), ("more layers", lambda d, p: rc_of(d.set_temporal_layers, 3, 0), ERR_STATE)], None),
    "a period, then a split": ({}, refresh_then_split, [("a frame", frame_call, ERR_STATE), ("another period", lambda d, p: rc_of(d.set_intra_refresh, 4), ERR_STATE)], None),
    "hidden alt-refs and a layer burnt in": ({}, arf_and_a_layer, [("a hidden frame", hidden_frame, ERR_ARG)], None),
    "hidden alt-refs and a denoiser behind them": ({}, lambda d: (arf_and_a_frame(d), d.set_denoise(1)), [("a hidden frame", hidden_frame, ERR_ARG)], None),
}


def walk(name, asked):
    from vp8oclenc_amd import api
    cfg, way_in, asks, feed = STATES[name]
    d = api.NativeDriver(W, H, **dict(GOOD, **cfg))
    way_out = way_in(d) if way_in else None
    if asked:
        partner = api.NativeDriver(W, H, **GOOD)
        before = bytes(d.stats())
        for what, ask, code in asks:
            assert ask(d, partner) == code, (name, what)
            assert bytes(d.stats()) == before, (name, what)
        partner.close()
    if callable(way_out):
        way_out()
    out = stream(d, 3, feed)
    d.close()
    return out


@pytest.mark.parametrize("name", sorted(STATES))
def test_a_state_refuses_with_its_code_and_nothing_has_moved(name):
    got, undisturbed = walk(name, True), walk(name, False)
    assert all(len(f) > 3 for f in got) and got == undisturbed


def test_the_partner_is_fit_for_a_batch():
    """the control of every `membership` above: two drivers of the partner's kind make a batch"""
    from vp8oclenc_amd import api
    a, b = api.NativeDriver(W, H, **GOOD), api.NativeDriver(W, H, **GOOD)
    assert batch_rc([a, b]) == 0 and batch_rc([a]) == 0
    a.close()
    b.close()


# ---- members must agree; a call that is wrong in two ways ---------------------------------------------------------------------------------
DIFFER = {"quantiser range": (dict(qi_max=50), None), "check_SSIM": (dict(check_ssim=0), None), "partitions": (dict(num_partitions=2), None),
          "filter type": (dict(loop_filter_type=1), None), "denoise level": ({}, lambda d: d.set_denoise(2)), "format": ({}, lambda d: d.set_source_format(I422)),
          "matrix": ({}, lambda d: d.set_source_colour(1)), "analysis": ({}, lambda d: d.set_analysis(True)), "deinterlace mode": ({}, lambda d: d.set_deinterlace(1, 0)),
          "parity": ({}, lambda d: d.set_deinterlace(1, 1)), "segment mode": ({}, lambda d: d.set_segment_mode(2, 2))}


@pytest.mark.parametrize("what", sorted(DIFFER))
def test_members_that_differ_make_no_batch_and_code_on(what):
    from vp8oclenc_amd import api
    cfg, setter = DIFFER[what]
    a, b = api.NativeDriver(W, H, **GOOD), api.NativeDriver(W, H, **dict(GOOD, **cfg))
    if what == "parity":
        a.set_deinterlace(1, 0)
    if setter:
        setter(b)
    assert batch_rc([a, b]) == ERR_ARG and batch_rc([b, a]) == ERR_ARG
    assert batch_rc([a]) == 0 and batch_rc([b]) == 0      # each on its own is fit
    a.close()
    b.close()


def test_a_member_of_another_batch_beside_one_that_differs_is_an_argument_error():
    """member 0 belongs to a live batch already (the context's ERR_STATE) and member 1 has another denoise level (ERR_ARG): the driver
    looks at every member's settings before the context looks at any member's state"""
    from vp8oclenc_amd import api
    a, b, c = (api.NativeDriver(W, H, **GOOD) for _ in range(3))
    c.set_denoise(2)
    first = api.NativeBatch([a, b])
    assert batch_rc([a, c]) == ERR_ARG
    c.set_denoise(0)
    assert batch_rc([a, c]) == ERR_STATE      # wrong in the one way only
    assert [d.stats().frame_number for d in (a, b, c)] == [0, 0, 0]
    got = []
    for t in range(3):
        first.encode_frame_host([tuple(p.ctypes.data for p in frames()[t]), tuple(p.ctypes.data for p in frames()[t + 1])])
        first.get_frames_begin()
        got.append([d.get_frame_end() for d in (a, b)])
    first.close()
    alone = []
    for k in range(2):
        d = api.NativeDriver(W, H, **GOOD)
        alone.append([(d.encode_frame_host(*frames()[t + k]), d.get_frame())[1] for t in range(3)])
        d.close()
    assert got == [list(x) for x in zip(*alone)]
    for d in (a, b, c):
        d.close()


# ---- the batched scan --------------------------------------------------------------------------------------------------------------------
SCAN = {"denoise": ({}, lambda d: d.set_denoise(2)), "deinterlace adaptive": ({}, lambda d: d.set_deinterlace(2, 0)), "analysis": ({}, lambda d: d.set_analysis(True)),
        "quality statistics": (dict(quality_stats=1), None)}


@pytest.mark.parametrize("what", sorted(SCAN))
def test_a_scan_is_refused_by_what_keeps_a_history(what):
    from vp8oclenc_amd import api
    cfg, setter = SCAN[what]
    planes = lambda t: [tuple(p.ctypes.data for p in frames()[t + i]) for i in range(2)]
    got = []
    for asked in (True, False):
        drivers = [api.NativeDriver(W, H, **dict(GOOD, **cfg)) for _ in range(2)]
        for d in drivers:
            if setter:
                setter(d)
        batch = api.NativeBatch(drivers)
        if asked:
            for host in (True, False):
                assert rc_of(batch.scan_frame_device, planes(0), None, host) == ERR_STATE
            assert [d.stats().frame_number for d in drivers] == [0, 0]
        out = []
        for t in range(3):
            batch.encode_frame_host(planes(t))
            batch.get_frames_begin()
            out.append([d.get_frame_end() for d in drivers])
        got.append(out)
        batch.close()
        for d in drivers:
            d.close()
    assert got[0] == got[1]
    # deinterlace mode 1 is a function of the one frame: scanned
    drivers = [api.NativeDriver(W, H, **GOOD) for _ in range(2)]
    for d in drivers:
        d.set_deinterlace(1, 0)
    batch = api.NativeBatch(drivers)
    assert rc_of(batch.scan_frame_device, planes(0), None, True) == 0 and len(batch.scan_result()) == 2
    batch.close()
    for d in drivers:
        d.close()


# ---- the record of the frame just coded -------------------------------------------------------------------------------------------------
def test_key_frames_of_a_batch_leave_the_record_of_key_frames_coded_alone():
    """GOPs of 2, 2 and 3 frames: call 0 codes three key frames in the batched launch, call 2 two of them beside an inter frame, call 3 a
    single key frame on the member's ordinary path beside two inter frames; after every call each member's statistics, layer record,
    refresh record and bytes are those of the same driver coded on its own"""
    from vp8oclenc_amd import api
    gops = (2, 2, 3)
    cfgs = [dict(GOOD, gop_size=g, altref_range=g + 1) for g in gops]

    def record(d, frame):
        return bytes(d.stats()), bytes(d.frame_layer()), bytes(d.intra_refresh()), frame

    alone = []
    for k, cfg in enumerate(cfgs):
        d = api.NativeDriver(W, H, **cfg)
        rec = []
        for t in range(5):
            key = d.encode_frame_host(*frames()[(t + k) % 6])
            rec.append((key,) + record(d, d.get_frame()))
        alone.append(rec)
        d.close()
    keys = [[r[0] for r in rec] for rec in alone]
    assert [k[2] for k in keys] == [True, True, False] and [k[3] for k in keys] == [False, False, True]      # the two branches are taken
    drivers = [api.NativeDriver(W, H, **cfg) for cfg in cfgs]
    batch = api.NativeBatch(drivers)
    for t in range(5):
        was_key = batch.encode_frame_host([tuple(p.ctypes.data for p in frames()[(t + k) % 6]) for k in range(3)])
        batch.get_frames_begin()
        for k, d in enumerate(drivers):
            frame = d.get_frame_end()
            assert record(d, frame) == alone[k][t][1:], (t, k)
            assert was_key[k] == (t % gops[k] == 0)
    batch.close()
    for d in drivers:
        d.close()
