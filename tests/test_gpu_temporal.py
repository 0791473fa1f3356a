"""Temporal layers on the device: the native driver with two and three layers against the CPU oracle's frame loop with the rule's
reference sets and refreshes (tests/temporal_ref.py) -- every frame's bytes, every reconstruction whichever buffer it went to or none,
every layer record -- and, on a conformant stream, against the RFC 6386 decoder of tests/vp8_decode.py: the whole stream and the
streams a forwarding unit makes of it by dropping the upper layers.  Skipping the filter of an unreferenced frame changes no byte;
key frames of every origin restart the pattern; a GOP coded as a chunk gives the serial bytes; both first-partition coders agree;
every refusal at both layers; off is off.  Everything is exact: no tolerances.
What the byte comparisons of GOLDEN-only and unreferenced frames prove: their expected first partition comes from the project's own
host coder (the reference writes no such header; tests/temporal_ref.record_bytes), so they hold the device coder to the host coder.
The independent judge of those bytes is the decoder: every conformant_stream = 1 case decodes them."""
import ctypes as C
import functools
import importlib.util
import os
import zlib

import numpy as np
import pytest

import arf_ref
import temporal_ref as ref

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QI = dict(qi_min=10, qi_max=60)
TOTAL, GOP = 13, 9      # a key frame at 9, where three layers would have put a temporal_id 2 frame (p = 9) and two a temporal_id 1 frame: p restarts
RANGE = GOP + 1         # cfg.altref_range above cfg.gop_size: no scheduled alt-refs


def same(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


@functools.lru_cache(maxsize=None)
def pan(w, h, total=TOTAL):
    return arf_ref.noisy_pan(w, h, total, seed=w + total)


@functools.lru_cache(maxsize=None)
def pan_with_a_cut(w, h, amplitude=5):
    """seven frames of one picture, six of another in other colours: a cut at frame 7 (p = 7: a temporal_id 2 frame of three layers).
    amplitude = 1: noise below scene_change()'s thresholds (mean chroma differences of 4 and 6 between neighbours, 40 at the cut)"""
    return arf_ref.noisy_pan(w, h, 7, seed=w + 7, amplitude=amplitude) + \
        [(y, 255 - u, 255 - v) for y, u, v in arf_ref.noisy_pan(w, h, 6, seed=5, amplitude=amplitude)]


@functools.lru_cache(maxsize=None)
def oracle_records(kind, w, h, layers, ref_mask, conformant, force_key=(), check=True, cfg=()):
    frames = pan(w, h) if kind == "pan" else pan_with_a_cut(w, h, 1 if kind == "calm cut" else 5)
    c = dict(gop_size=GOP, altref_range=RANGE, **QI)
    c.update(dict(cfg))
    return frames, ref.oracle_loop(frames, layers, conformant=bool(conformant), force_key=frozenset(force_key), ref_mask=ref_mask, check_ssim=check, **c)


@functools.lru_cache(maxsize=None)
def expected_bytes(key, i, P):
    frames, recs = oracle_records(*key)
    h, w = frames[0][0].shape
    return ref.record_bytes(recs[i], w, h, P)


def layer_tuple(x):
    get = (lambda k: x[k]) if isinstance(x, dict) else (lambda k: getattr(x, k))
    return tuple(int(get(k)) for k in ("temporal_id", "tl0_pic_idx", "layer_sync", "refresh", "use_golden"))


def run_driver(key, P, layers, way="host", decode=False, flags=1, force_key=(), compare=True, first=0, **cfg):
    """the native driver over the records' frames from `first` on -> dict(stream, infos, keys, recons); asserts bytes, reconstructions,
    layer records and the reference count frame by frame"""
    from vp8oclenc_amd import api
    frames, recs = oracle_records(*key)
    h, w = frames[0][0].shape
    c = dict(gop_size=GOP, altref_range=RANGE, num_partitions=P, check_ssim=1, **QI)
    c.update(cfg)
    drv = api.NativeDriver(w, h, **c)
    drv.set_temporal_layers(layers, flags)
    dec = None
    if decode:
        import vp8_decode
        dec = vp8_decode.Decoder()
    dev = [[api.to_device(p) for p in f] for f in frames] if way == "device" else None
    if dev:
        api.device_synchronize()
    seen = dict(stream=[], infos=[], keys=[], recons=[], pictures=[])
    base = None
    for t in range(first, len(frames)):
        r, what = recs[t], f"frame {t}"
        searched = drv.stats().refs_searched
        fk = t in force_key or t == first and first > 0
        if dev:
            was_key = drv.encode_frame_device(*(b.data_ptr() for b in dev[t]), force_key=fk)
        else:
            was_key = drv.encode_frame_host(*frames[t], force_key=fk)
        got = drv.get_frame()
        was_key = drv.resolve() or was_key
        info = drv.frame_layer()
        assert bool(was_key) == r["key"], what
        assert got[0] & 0x10 and (got[0] & 1) == (not r["key"]), what      # shown; key / inter
        if compare:
            assert layer_tuple(info) == layer_tuple(r["layer"]), (what, layer_tuple(info), layer_tuple(r["layer"]))
            exp = expected_bytes(key, t, P)
            assert len(got) == len(exp), f"{what}: {len(got)} bytes, expected {len(exp)}"
            if got != exp:
                a, b = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
                raise AssertionError(f"{what} differs at bytes {np.nonzero(a != b)[0][:8]} of {len(a)}")
        if not r["key"] and not r.get("sent_back"):
            assert drv.stats().refs_searched - searched == 1 + info.use_golden, what
        last = drv.hip.download_last()
        if info.refresh in (ref.LAST, ref.ALL):
            base = recon = last
        else:
            same(last, base, what + ": LAST behind a frame that does not refresh it")
            recon = drv.hip.refresh_frame() if info.filtered else None
        if compare and recon is not None:
            same(recon, r["recon"], what)
        if dec is not None:
            before = dict(dec.ref) if getattr(dec, "ref", None) else {}
            f, planes = dec.decode(got)
            same(planes, recon, what + ": the decoder against the device")
            if info.refresh == ref.GOLDEN:
                assert dec.ref[1] is before[1] and dec.ref[2] is planes and dec.ref[3] is before[3], what
            elif info.refresh == ref.NONE:
                assert all(dec.ref[k] is before[k] for k in (1, 2, 3)), what
            seen["pictures"].append(planes)
        seen["stream"].append(got)
        seen["infos"].append(info)
        seen["keys"].append(bool(was_key))
        seen["recons"].append(recon)
    seen["stats"] = drv.stats()
    drv.close()
    for f in dev or ():
        for b in f:
            b.free()
    return seen


# ---- 5. the driver against the oracle's loop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conformant", [0, 1])
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("ref_mask", [3, 0])
@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("w,h", [(64, 48), (96, 64)])
def test_a_layered_driver_equals_the_oracle_loop(w, h, layers, ref_mask, P, conformant):
    """bytes, reconstructions (VP8DRV_TL_KEEP_RECON: the unreferenced ones too) and layer records of 13 frames, device intake with four
    partitions and host intake with one; fails on a tree without temporal layers (there is no setter)"""
    key = ("pan", w, h, layers, ref_mask, conformant)
    seen = run_driver(key, P, layers, way="device" if P == 4 else "host", decode=bool(conformant), ref_mask=ref_mask, conformant_stream=conformant)
    assert seen["keys"] == [t in (0, GOP) for t in range(TOTAL)]
    assert [i.temporal_id for i in seen["infos"]] == [r["temporal_id"] for r in ref.records(layers, {GOP}, TOTAL, ref_mask)]
    assert all(i.filtered for i in seen["infos"])
    if layers == 3:
        assert any(i.refresh == ref.GOLDEN for i in seen["infos"]) and any(i.use_golden for i in seen["infos"]) == bool(ref_mask & 1)


# ---- 6. the sub-streams decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_the_streams_without_the_upper_layers_decode_to_the_same_pictures(layers):
    import vp8_decode
    w, h = 96, 64
    seen = run_driver(("pan", w, h, layers, 3, 1), 2, layers, decode=True, conformant_stream=1)
    tids = [i.temporal_id for i in seen["infos"]]
    assert set(tids) == set(range(layers))
    for K in (1, 0):
        dec = vp8_decode.Decoder()
        kept = 0
        for t, (b, tid) in enumerate(zip(seen["stream"], tids)):
            if tid > K:
                continue
            _, planes = dec.decode(b)
            same(planes, seen["pictures"][t], f"layers <= {K}: frame {t}")
            kept += 1
        assert kept == sum(tid <= K for tid in tids) and (kept < TOTAL or K + 1 >= layers)


# ---- 7. skipping the filter changes no byte ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_an_unreferenced_frame_that_nobody_reads_is_not_filtered_and_no_byte_changes(layers):
    w, h = 64, 48
    key = ("pan", w, h, layers, 3, 0, (), False)      # (the oracle loop without check_SSIM)
    kept = run_driver(key, 2, layers, flags=1, check_ssim=0)
    bare = run_driver(key, 2, layers, flags=0, check_ssim=0)      # (LAST behind every such frame is the last temporal_id 0 frame's: run_driver)
    assert kept["stream"] == bare["stream"]
    assert all(i.filtered for i in kept["infos"])
    assert [i.filtered for i in bare["infos"]] == [int(i.refresh != ref.NONE) for i in bare["infos"]] and not all(i.filtered for i in bare["infos"])
    # ... and each of the things that read the filter's output, or ride in its launch, brings it back
    for cfg, setter in ((dict(check_ssim=1), None), (dict(check_ssim=0, quality_stats=1), None), (dict(check_ssim=0), "analysis")):
        from vp8oclenc_amd import api
        drv = api.NativeDriver(w, h, gop_size=GOP, altref_range=RANGE, **QI, **cfg)
        drv.set_temporal_layers(layers, 0)
        if setter:
            drv.set_analysis(True)
        for t in range(3):
            drv.encode_frame_host(*pan(w, h)[t])
            drv.resolve()
            assert drv.frame_layer().filtered == 1, (cfg, setter, t)
        drv.close()


# ---- 8. the layer records, whoever asks for a key frame ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_a_forced_key_frame_restarts_the_pattern(layers):
    key = ("pan", 64, 48, layers, 3, 1, (6,))
    seen = run_driver(key, 1, layers, decode=True, force_key=(6,), conformant_stream=1)
    assert seen["keys"] == [t in (0, 6) for t in range(TOTAL)]      # (the schedule's next key frame is nine frames behind the forced one)
    assert [layer_tuple(i) for i in seen["infos"]] == [layer_tuple(r) for r in ref.records(layers, {6}, TOTAL)]


def test_a_scene_cut_restarts_the_pattern():
    from vp8oclenc_amd import api
    w, h, layers = 64, 48, 3
    frames = pan_with_a_cut(w, h, 1)
    drv = api.NativeDriver(w, h, gop_size=150, altref_range=151, scene_detect=1, **QI)
    drv.set_temporal_layers(layers, 0)
    keys, infos = [], []
    for f in frames:
        k = drv.encode_frame_host(*f)
        keys.append(bool(drv.resolve() or k))
        infos.append(drv.frame_layer())
    assert keys == [t in (0, 7) for t in range(TOTAL)] and drv.stats().scene_changes == 1
    drv.close()
    assert [layer_tuple(i) for i in infos] == [layer_tuple(r) for r in ref.records(layers, {7}, TOTAL)]
    # the same bytes as a stream whose key frame at the cut was asked for by the caller
    cfg = (("gop_size", 150), ("altref_range", 151))
    seen = run_driver(("calm cut", w, h, layers, 3, 0, (7,), True, cfg), 1, layers, flags=0, gop_size=150, altref_range=151, scene_detect=1)
    assert seen["keys"] == keys and seen["stats"].scene_changes == 1


def test_a_frame_sent_back_by_check_ssim_restarts_the_pattern():
    """quantisers and a target from the range of tests/test_gpu_check_async.py's cases, at which the frame behind the cut -- p = 7, an
    unreferenced temporal_id 2 frame that searches GOLDEN -- has more than a sixth of its macroblocks replaced and is coded again as a key
    frame, and other frames have macroblocks replaced and stay inter frames (their headers carry intra modes)"""
    w, h, layers = 96, 64, 3
    cfg = (("gop_size", 150), ("altref_range", 151), ("qi_min", 40), ("qi_max", 110), ("ssim_target", 0.90))
    key = ("cut", w, h, layers, 3, 0, (), True, cfg)
    frames, recs = oracle_records(*key)
    assert recs[0]["redone_as_key"] == 1 and [r["key"] for r in recs] == [t in (0, 7) for t in range(TOTAL)]
    assert any(r["out"].get("replaced", 0) > 0 and r["layer"]["refresh"] != ref.LAST for r in recs if not r["key"])
    recs[7]["sent_back"] = True
    seen = run_driver(key, 2, layers, **dict(cfg))
    assert seen["stats"].redone_as_key == 1 and seen["stats"].key_frames == 2
    assert [layer_tuple(i) for i in seen["infos"]] == [layer_tuple(r) for r in ref.records(layers, {7}, TOTAL)]


# ---- 9. GOP chunks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_a_gop_coded_as_a_chunk_gives_the_serial_bytes(layers):
    key = ("pan", 64, 48, layers, 3, 0)
    serial = run_driver(key, 2, layers)
    chunk = run_driver(key, 2, layers, first=GOP, compare=False)      # a fresh driver, its first frame with force_key
    assert chunk["keys"] == [True, False, False, False]
    assert chunk["stream"] == serial["stream"][GOP:]
    assert [layer_tuple(i)[0] for i in chunk["infos"]] == [layer_tuple(i)[0] for i in serial["infos"][GOP:]]
    for a, b in zip(chunk["recons"], serial["recons"][GOP:]):
        same(a, b, "chunk")


# ---- 10. the two first-partition coders ------------------------------------------------------------------------------------------------------
def test_device_and_host_first_partitions_agree_on_layered_frames():
    key = ("pan", 96, 64, 3, 3, 0)
    streams = [run_driver(key, 2, 3, host_bitstream=hb) for hb in (0, 1)]
    assert streams[0]["stream"] == streams[1]["stream"]
    refreshes = [i.refresh for i in streams[1]["infos"]]
    assert ref.GOLDEN in refreshes and ref.NONE in refreshes


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_driver_and_nothing_has_changed():
    from vp8oclenc_amd import api, ref_shard
    w, h = 64, 48
    frames = pan(w, h)
    lib = api.load_library()
    lib.vp8drv_set_temporal_layers.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8drv_get_frame_layer.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8drv_set_arf.argtypes = [C.c_void_p, C.c_int]
    lib.vp8hip_shard_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    lib.vp8drv_encode_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    good = dict(gop_size=GOP, altref_range=RANGE, **QI)
    info = api.LayerInfo()

    def stream(drv, n=5):
        out = []
        for t in range(n):
            drv.encode_frame_host(*frames[t])
            out.append(drv.get_frame())
            drv.resolve()
        return out

    plain = api.NativeDriver(w, h, **good)
    undisturbed = stream(plain)
    plain.close()
    # the arguments; scheduled alt-refs; hidden alt-refs, both ways round
    drv = api.NativeDriver(w, h, **good)
    assert lib.vp8drv_get_frame_layer(drv.h, C.byref(info)) == ERR_STATE      # no frame coded yet
    for layers, flags in ((0, 0), (4, 0), (-1, 0), (2, 2), (3, -1)):
        assert lib.vp8drv_set_temporal_layers(drv.h, layers, flags) == ERR_ARG, (layers, flags)
    assert lib.vp8drv_set_temporal_layers(None, 2, 0) == ERR_ARG and lib.vp8drv_get_frame_layer(drv.h, None) == ERR_ARG
    assert lib.vp8drv_set_arf(drv.h, 4) == 0
    assert lib.vp8drv_set_temporal_layers(drv.h, 2, 0) == ERR_STATE
    assert lib.vp8drv_set_temporal_layers(drv.h, 1, 0) == 0                  # (off is always accepted)
    assert lib.vp8drv_set_arf(drv.h, 0) == 0
    # a member of a live batch
    other = api.NativeDriver(w, h, **good)
    batch = api.NativeBatch([drv, other])
    assert lib.vp8drv_set_temporal_layers(drv.h, 3, 0) == ERR_STATE
    batch.close()
    other.close()
    assert stream(drv) == undisturbed      # after all of them: an undisturbed driver's bytes
    assert lib.vp8drv_get_frame_layer(drv.h, C.byref(info)) == 0 and (info.temporal_id, info.refresh, info.filtered) == (0, ref.LAST, 1)
    drv.close()
    # ... and the other way round: with layers asked for, hidden alt-refs and a batch are refused
    drv = api.NativeDriver(w, h, **good)
    drv.set_temporal_layers(3, 0)
    assert lib.vp8drv_set_arf(drv.h, 4) == ERR_STATE
    other = api.NativeDriver(w, h, **good)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch([drv, other])
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch([other, drv])
    other.close()
    layered = stream(drv)
    drv.close()
    key = ("pan", w, h, 3, 3, 0)
    assert layered == [expected_bytes(key, t, 1) for t in range(5)]      # ... and the layered stream is the oracle loop's
    # the configuration: scheduled alt-refs on (the default altref_range), the overlapped filter, the host parameter mirror
    for cfg in (dict(good, altref_range=GOP), dict(gop_size=GOP, **QI), dict(good, overlap_filter=1), dict(good, device_params=0)):
        d = api.NativeDriver(w, h, **cfg)
        for layers in (2, 3):
            assert lib.vp8drv_set_temporal_layers(d.h, layers, 1) == ERR_ARG, cfg
        assert lib.vp8drv_set_temporal_layers(d.h, 1, 0) == 0
        d.close()
    # a by-reference split (vp8hip_shard_init; one rank is enough to make it one) joined behind the setter: the frame calls, and the setter again
    drv = api.NativeDriver(w, h, **good)
    drv.set_temporal_layers(2, 0)
    assert stream(drv, 1) == undisturbed[:1]
    last = [p.copy() for p in drv.hip.download_last()]
    assert lib.vp8hip_shard_init(drv.hip.h, ref_shard.shard_unique_id(), 0, 1) == 0
    y, u, v = (np.ascontiguousarray(p) for p in frames[1])
    assert lib.vp8drv_encode_frame_host(drv.h, y.ctypes.data, u.ctypes.data, v.ctypes.data, 0) == ERR_STATE
    assert lib.vp8drv_set_temporal_layers(drv.h, 3, 1) == ERR_STATE
    assert drv.stats().frame_number == 1
    same(drv.hip.download_last(), last, "LAST after the refusals")
    assert lib.vp8drv_set_temporal_layers(drv.h, 1, 0) == 0      # off is accepted, and the split's own frame calls are the split's business again
    drv.close()


def test_every_refusal_of_the_context():
    from vp8oclenc_amd import api, ref_shard
    w, h = 64, 48
    frames = pan(w, h)
    lib = api.load_library()
    lib.vp8hip_loop_filter_refresh.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8hip_shard_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    refqi, _ = api.quantizer_ladders(10, 60)

    def key_frame(hip):
        hip.upload_current(*frames[0])
        hip.auto_segments(True, refqi, 10)
        hip.intra_transform()
        hip.prepare_filter_mask(want_nz=False)

    def inter_frame(hip, t=1, rotate=1):
        hip.upload_current(*frames[t])
        hip.auto_segments(False, refqi, 10)
        hip.inter_transform(rotate, rotate, 0, 0)

    hip = api.Vp8Hip(w, h)
    for refresh, filt in ((3, 1), (-1, 1), (ref.NONE, 2), (ref.NONE, -1), (ref.GOLDEN, 0), (ref.LAST, 0)):
        assert lib.vp8hip_loop_filter_refresh(hip.h, refresh, filt) == ERR_ARG, (refresh, filt)
    assert lib.vp8hip_loop_filter_refresh(None, ref.NONE, 1) == ERR_ARG
    for refresh, filt in ((ref.LAST, 1), (ref.GOLDEN, 1), (ref.NONE, 1), (ref.NONE, 0)):
        assert lib.vp8hip_loop_filter_refresh(hip.h, refresh, filt) == ERR_STATE      # no reconstruction
    key_frame(hip)
    for refresh, filt in ((ref.GOLDEN, 1), (ref.NONE, 1), (ref.NONE, 0)):
        assert lib.vp8hip_loop_filter_refresh(hip.h, refresh, filt) == ERR_STATE      # a key frame refreshes everything
    hip.loop_filter_refresh(ref.LAST)                                                  # ... which is vp8hip_loop_filter
    key_recon = [p.copy() for p in hip.download_last()]
    # an armed check_SSIM: its verdict rides in the filter's launch, so the ending without a filter refuses it and the one with carries it
    inter_frame(hip)
    hip.check_ssim_async(refqi, 10)
    assert lib.vp8hip_loop_filter_refresh(hip.h, ref.NONE, 0) == ERR_STATE
    hip.loop_filter_refresh(ref.NONE, True)
    assert hip.check_ssim_result()[0] == 0
    same(hip.download_last(), key_recon, "LAST behind a dropped frame")
    # the filter beside the next frame (vp8hip_filter_overlap)
    inter_frame(hip, 2, 0)
    hip.filter_overlap(True)
    for refresh, filt in ((ref.GOLDEN, 1), (ref.NONE, 1), (ref.NONE, 0)):
        assert lib.vp8hip_loop_filter_refresh(hip.h, refresh, filt) == ERR_STATE
    hip.filter_overlap(False)
    hip.loop_filter_refresh(ref.GOLDEN)
    same(hip.download_last(), key_recon, "LAST behind a GOLDEN-only frame")
    golden = hip.refresh_frame()
    assert any(not np.array_equal(a, b) for a, b in zip(golden, key_recon))
    hip.close()
    # a by-reference split, and a member of a live batch
    be = ref_shard.HipRefBackend(w, h)
    key_frame(be)
    be.loop_filter()
    inter_frame(be)
    be.shard_init(ref_shard.shard_unique_id(), 0, 1)
    for refresh, filt in ((ref.GOLDEN, 1), (ref.NONE, 1), (ref.NONE, 0)):
        assert lib.vp8hip_loop_filter_refresh(be.h, refresh, filt) == ERR_STATE
    be.close()
    ctxs = [api.Vp8Hip(w, h), api.Vp8Hip(w, h)]
    for c in ctxs:
        key_frame(c)
        c.loop_filter()
        inter_frame(c)
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    hb = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * 2)(ctxs[0].h, ctxs[1].h), 2) == 0
    for c in ctxs:
        for refresh, filt in ((ref.GOLDEN, 1), (ref.NONE, 1), (ref.NONE, 0)):
            assert lib.vp8hip_loop_filter_refresh(c.h, refresh, filt) == ERR_STATE
    lib.vp8hip_batch_destroy(hb)
    ctxs[0].loop_filter_refresh(ref.GOLDEN)      # on its own again it ends the frame
    for c in ctxs:
        c.close()


# ---- 12. off is off ----------------------------------------------------------------------------------------------------------------------------
def test_off_by_default_the_committed_sequence_keeps_its_bytes():
    """a driver that never calls the new entry points, and one that calls vp8drv_set_temporal_layers(1, 0), on the small sequence whose
    digests are committed (tests/golden/full_length/selftest.json): every frame's bytes and every reconstruction"""
    from vp8oclenc_amd import api
    from vp8oclenc_amd.synth import bench_frames
    spec = importlib.util.spec_from_file_location("full_length_oracle", os.path.join(ROOT, "scripts", "full_length_oracle.py"))
    flo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(flo)
    doc = flo.load("selftest")
    W0, H0 = doc["source"]
    W, H, source, _ = bench_frames(W0, H0, doc["seed"], flo.ND)
    cfg = dict(altref_range=flo.ALTREF_RANGE, qi_min=0, qi_max=48, ssim_target=-1.0, device_params=1, check_ssim=1, src_width=W0, src_height=H0,
               gop_size=doc["gop"])
    for call in (False, True):
        d = api.NativeDriver(W, H, **cfg)
        if call:
            d.set_temporal_layers(1, 0)
        for t in range(doc["frames"]):
            d.encode_frame_host(*source[t % flo.ND])
            b = d.get_frame()
            d.resolve()
            assert (zlib.crc32(b), len(b)) == (doc["frame_crc32"][t], doc["frame_len"][t]), (call, t)
            assert flo.crc_planes(d.hip.download_last()) == doc["recon_crc32"][t], (call, t)
            info = d.frame_layer()
            assert (info.temporal_id, info.tl0_pic_idx, info.layer_sync, info.filtered) == (0, t & 255, 0, 1), (call, t)
        d.close()


@pytest.mark.parametrize("turn", ["off", "on"])
def test_a_layer_count_set_inside_a_gop_takes_force_at_the_next_key_frame(turn):
    """documented in include/vp8hip_driver.h: the count is in force from the next key frame on, so a receiver never sees half a pattern.
    Set at frame 5 of a GOP of 9: frames 5 .. 8 are still those of the stream as it was, frames 9 .. 12 those of the other stream (a GOP is
    closed: a plain stream's second GOP does not depend on how the first was coded, nor does a layered one's)"""
    from vp8oclenc_amd import api
    w, h, layers = 64, 48, 3
    frames = pan(w, h)
    key = ("pan", w, h, layers, 3, 0)
    layered = run_driver(key, 1, layers, flags=0)["stream"]
    plain = run_driver(key, 1, 1, flags=0, compare=False)["stream"]
    assert plain[0] == layered[0] and plain[1] != layered[1]
    drv = api.NativeDriver(w, h, gop_size=GOP, altref_range=RANGE, **QI)
    if turn == "off":
        drv.set_temporal_layers(layers, 0)
    got, tids = [], []
    for t, f in enumerate(frames):
        if t == 5:
            drv.set_temporal_layers(1 if turn == "off" else layers, 0)
        drv.encode_frame_host(*f)
        got.append(drv.get_frame())
        drv.resolve()
        tids.append(drv.frame_layer().temporal_id)
    drv.close()
    before, after = (layered, plain) if turn == "off" else (plain, layered)
    assert got[:GOP] == before[:GOP] and got[GOP:] == after[GOP:]
    want = [r["temporal_id"] for r in ref.records(layers, {GOP}, TOTAL)]
    assert tids == (want[:GOP] + [0] * 4 if turn == "off" else [0] * GOP + want[GOP:])
