"""Hidden alternate reference frames on the device: k_arf_filter_b against the numpy restatement of tests/arf_ref.py byte for byte
whichever way the window comes in and whatever the intake does to the filtered frame afterwards; the native driver with hidden frames
against the CPU oracle's frame loop with the same hidden frames (bytes and reconstructions, hidden ones included) and, on a conformant
stream, against the RFC 6386 decoder of tests/vp8_decode.py; the reference-rotation hazard; both first-partition coders; every refusal;
off is off.  Everything is exact: no tolerances.
What the byte comparisons of HIDDEN frames prove: their expected first partition comes from the project's own host coder (the reference
has no such frame; tests/arf_ref.record_bytes), so they hold the device coder to the host coder, and with host_bitstream = 1 the code to
itself.  The independent judge of a hidden frame's bytes is the decoder: every conformant_stream = 1 case decodes each record with
tests/vp8_decode.py and compares it with the device's reconstruction."""
import ctypes as C
import functools
import importlib.util
import os
import zlib

import numpy as np
import pytest

import arf_ref as ref

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (64, 48), (40, 24), (56, 40)]


def same(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


@functools.lru_cache(maxsize=None)
def restated(w, h, n, centre, strength, seed):
    frames = ref.wild(w, h, n, seed=seed)
    return (frames,) + ref.filter_frame(frames, centre, strength)


def current_surfaces(hip):
    from vp8oclenc_amd import api
    return (hip.debug(api.DBG_PYRAMID, 3, 0), hip.debug(api.DBG_CURRENT_CHROMA, 0), hip.debug(api.DBG_CURRENT_CHROMA, 1))


def filter_on_device(hip, frames, centre, strength, way):
    from vp8oclenc_amd import api
    if way == "host":
        return hip.arf_filter(frames, centre, strength)
    dev = [[api.to_device(p) for p in f] for f in frames]      # vp8hip_device_alloc memory, one allocation per plane
    hip.arf_filter_device([tuple(b.data_ptr() for b in f) for f in dev], centre, strength)
    out = hip.arf_frame()      # (blocks: the planes may go)
    for f in dev:
        for b in f:
            b.free()
    return out


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["device", "host"])
@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_equals_the_restatement_byte_for_byte(w, h, way):
    from vp8oclenc_amd import api
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    hip = api.Vp8Hip(W, H)
    if (w, h) != (W, H):
        hip.set_source_size(w, h)
    tiles = (W // 16) * (H // 16)
    for n in (1, 3, 7):
        for centre in sorted({0, n // 2, n - 1}):
            for strength in (0, 3, 6):
                frames, want, weights, _ = restated(w, h, n, centre, strength, w + n)
                got = filter_on_device(hip, frames, centre, strength, way)
                same(got, want, f"n {n} centre {centre} strength {strength}")
                assert hip.arf_result() == weights and sum(weights) == tiles * (n - 1)
                if n == 1:
                    same(got, frames[0], "n = 1 returns the centre frame")
    hip.close()


@pytest.mark.parametrize("coded,src,scaled", [((64, 48), (56, 40), None), ((64, 48), None, (128, 96))])
def test_the_filtered_frame_passes_through_the_intake_like_a_source_frame(coded, src, scaled):
    """a source size below the coded size, and a scaler: the current frame behind the filter is the current frame of a context that was
    handed the restatement's frame"""
    from vp8oclenc_amd import api
    W, H = coded
    iw, ih = scaled or src
    plain, arf = api.Vp8Hip(W, H), api.Vp8Hip(W, H)
    for hip in (plain, arf):
        if scaled:
            hip.set_source_scaling(iw, ih, W, H, api.SCALE_AREA)
        else:
            hip.set_source_size(*src)
    for way in ("device", "host"):
        frames, want, weights, _ = restated(iw, ih, 5, 2, 3, 11)
        got = filter_on_device(arf, frames, 2, 3, way)
        same(got, want, "as it left the filter")
        plain.upload_current(*want)
        cur = current_surfaces(arf)
        assert cur[0].shape == (H, W)
        same(cur, current_surfaces(plain), f"current frame ({way})")
    plain.close()
    arf.close()


# ---- 2. the driver against the oracle's loop ------------------------------------------------------------------------------------------------
QI = dict(qi_min=10, qi_max=60)


@functools.lru_cache(maxsize=None)
def oracle_records(w, h, total, gop, placement, ref_mask, conformant, altref_range=5, strength=3):
    frames = ref.noisy_pan(w, h, total, seed=w + total)
    recs = ref.oracle_loop(frames, dict(placement), strength, conformant=bool(conformant), gop_size=gop, altref_range=altref_range, ref_mask=ref_mask, **QI)
    return frames, recs


def hidden_recon(drv):
    from vp8oclenc_amd import api
    return tuple(drv.hip.debug(api.DBG_ARF_FRAME, r) for r in (3, 4, 5))


def run_driver(frames, recs, P, strength=3, way="host", decode=False, stop_after=None, **cfg):
    """the native driver through the records' order of calls -> what it saw; asserts bytes and reconstructions record by record"""
    from vp8oclenc_amd import api
    h, w = frames[0][0].shape
    drv = api.NativeDriver(w, h, num_partitions=P, check_ssim=1, **cfg)
    drv.set_arf(strength + 1)
    dec = None
    if decode:
        import vp8_decode
        dec = vp8_decode.Decoder()
    seen = dict(hidden=0, altref_mbs=0, stream=[])
    dev, off = None, False
    if way == "device":
        dev = [[api.to_device(p) for p in f] for f in frames]
    for i, r in enumerate(recs):
        what = f"record {i} ({r['kind']} at frame {r['t']})"
        if r["kind"] == "hidden":
            if off:      # turned off behind an earlier hidden frame: refused, and on again
                with pytest.raises(api.Vp8HipError):
                    drv.encode_arf_host(frames[:1], 0)
                drv.set_arf(strength + 1)
                off = False
            lo, n, centre = r["window"]
            if way == "device":
                drv.encode_arf_device([tuple(b.data_ptr() for b in f) for f in dev[lo:lo + n]], centre)
            else:
                drv.encode_arf_host(frames[lo:lo + n], centre)
            got = drv.get_frame()
            recon = hidden_recon(drv)
            st = drv.arf_stats()
            seen["hidden"] += 1
            assert (st.hidden_frames, st.last_frames, list(st.last_weight)) == (seen["hidden"], n, r["weights"]), what
            assert (st.last_use_golden, st.last_use_altref) == (r["out"]["use_golden"], r["out"]["use_altref"]), what
            assert not got[0] & 0x10 and got[0] & 1, what      # an inter frame that is not shown
            if stop_after is not None and seen["hidden"] == stop_after:
                drv.set_arf(0)      # (the frames behind it still find the hidden frame in ALTREF)
                off = True
        else:
            was_key = drv.encode_frame_host(*frames[r["t"]])
            got = drv.get_frame()
            was_key = drv.resolve() or was_key
            assert bool(was_key) == r["key"], what
            recon = drv.hip.download_last()
            assert got[0] & 0x10, what
        exp = ref.record_bytes(r, w, h, P)
        assert len(got) == len(exp), f"{what}: {len(got)} bytes, expected {len(exp)}"
        if got != exp:
            a, b = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
            raise AssertionError(f"{what} differs at bytes {np.nonzero(a != b)[0][:8]} of {len(a)}")
        same(recon, r["recon"], what)
        if dec is not None:
            last_before = dec.ref.get(1) if getattr(dec, "ref", None) else None
            f, planes = dec.decode(got)
            same(planes, recon, what + ": the decoder against the device")
            if r["kind"] == "hidden":
                assert dec.ref[1] is last_before and dec.ref[3] is planes
            elif not r["key"]:
                seen["altref_mbs"] += int((f.ref_frame[f.is_inter.astype(bool)] == 3).sum())
        seen["stream"].append(got)
    st = drv.stats()
    shown = [r for r in recs if r["kind"] == "shown"]
    assert st.frame_number == len(shown) and st.key_frames + st.inter_frames == len(shown)      # hidden frames are not counted
    drv.close()
    return seen


@pytest.mark.parametrize("conformant", [0, 1])
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("ref_mask", [3, 0])
@pytest.mark.parametrize("w,h", [(64, 48), (96, 64)])
def test_a_driver_with_hidden_frames_equals_the_oracle_loop(w, h, ref_mask, P, conformant):
    total, gop, period = 12, 12, 4
    placement = ref.schedule(total, gop, period)
    frames, recs = oracle_records(w, h, total, gop, tuple(sorted(placement.items())), ref_mask, conformant)
    seen = run_driver(frames, recs, P, decode=bool(conformant), way="device" if P == 4 else "host", gop_size=gop, altref_range=5, ref_mask=ref_mask,
                      conformant_stream=conformant, **QI)
    assert seen["hidden"] == 3
    if conformant and ref_mask == 3:
        assert seen["altref_mbs"] > 0      # the shown frames use the hidden frame


# ---- 3. the rotation hazard -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["behind a key frame", "behind a scheduled alt-ref", "two in a row"])
def test_the_rotation_owed_is_applied_once(where):
    """the hidden frame's transform consumes the rotation the last shown frame owes; applied again by the next shown frame LAST
    would overwrite the new ALTREF -- the next frames' bytes and reconstructions would leave the oracle loop's"""
    w, h, total, gop = 64, 48, 9, 6      # a key frame at 0 and at 6; altref_range 3: shown alt-refs at 3 and (second GOP) none
    if where == "behind a key frame":
        placement = {0: (0, 4, 3, "after"), 6: (6, 3, 2, "after")}
    elif where == "behind a scheduled alt-ref":
        placement = {3: (1, 5, 3, "after"), 5: (3, 3, 2, "before")}
    else:
        placement = {2: (0, 5, 2, "before"), 3: (1, 5, 3, "after"), 4: (2, 4, 2, "before")}      # (... and hidden frames on both sides of the alt-ref at 3)
    frames, recs = oracle_records(w, h, total, gop, tuple(sorted(placement.items())), 3, 1, altref_range=3)
    kinds = [(r["kind"], r["t"]) for r in recs]
    if where == "two in a row":
        assert kinds[5:7] == [("hidden", 3), ("hidden", 4)]
    seen = run_driver(frames, recs, 2, decode=True, gop_size=gop, altref_range=3, ref_mask=3, conformant_stream=1, **QI)
    assert seen["hidden"] == len(placement) and seen["altref_mbs"] > 0


# ---- 4. the two first-partition coders --------------------------------------------------------------------------------------------------------
def test_device_and_host_first_partitions_agree_on_a_hidden_frame():
    w, h, total, gop = 96, 64, 6, 6
    placement = ref.schedule(total, gop, 3)
    frames, recs = oracle_records(w, h, total, gop, tuple(sorted(placement.items())), 3, 0)
    streams = [run_driver(frames, recs, 2, gop_size=gop, altref_range=5, ref_mask=3, host_bitstream=hb, **QI)["stream"] for hb in (0, 1)]
    assert streams[0] == streams[1] and sum(1 for f in streams[0] if not f[0] & 0x10) == 2


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal():
    from vp8oclenc_amd import api
    w, h = 64, 48
    frames = ref.noisy_pan(w, h, 3, seed=1)
    lib = api.load_library()
    lib.vp8drv_set_arf.argtypes = [C.c_void_p, C.c_int]
    lib.vp8drv_encode_arf_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.vp8drv_get_arf_stats.argtypes = [C.c_void_p, C.c_void_p]
    keep, table = api._plane_table(frames)
    st = api.ArfStats()

    def arf(drv, n=3, centre=1):
        return lib.vp8drv_encode_arf_host(drv.h, table, n, centre)

    drv = api.NativeDriver(w, h)
    assert arf(drv) == ERR_STATE                                   # hidden frames off
    assert lib.vp8drv_set_arf(drv.h, 8) == ERR_ARG and lib.vp8drv_set_arf(drv.h, -1) == ERR_ARG      # strength
    assert lib.vp8drv_set_arf(drv.h, 4) == 0
    assert arf(drv) == ERR_STATE                                   # no reference yet
    assert lib.vp8drv_get_arf_stats(drv.h, C.byref(st)) == ERR_STATE
    drv.encode_frame_host(*frames[0])
    for n, centre in ((0, 0), (8, 0), (3, 3), (3, -1)):
        assert arf(drv, n, centre) == ERR_ARG, (n, centre)
    assert lib.vp8drv_encode_arf_host(drv.h, None, 3, 1) == ERR_ARG
    hole = (C.c_void_p * 9)(*table)
    hole[4] = None
    assert lib.vp8drv_encode_arf_host(drv.h, hole, 3, 1) == ERR_ARG      # a null plane
    # what keeps a history, or reads frames another way, is refused with the switch on, and switching on is refused with it
    for on, off in ((lambda: drv.set_denoise(2), lambda: drv.set_denoise(0)), (lambda: drv.set_deinterlace(1, 0), lambda: drv.set_deinterlace(0, 0)),
                    (lambda: drv.set_analysis(True), lambda: drv.set_analysis(False)), (lambda: drv.set_source_format(1), lambda: drv.set_source_format(0))):
        on()
        assert arf(drv) == ERR_ARG
        assert lib.vp8drv_set_arf(drv.h, 4) == ERR_ARG
        off()
    lib.vp8drv_set_source_window.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    pitch = (C.c_int32 * 3)(w + 16, w // 2 + 8, w // 2 + 8)
    assert lib.vp8drv_set_source_window(drv.h, pitch, 0, 0) == 0
    assert arf(drv) == ERR_ARG and lib.vp8drv_set_arf(drv.h, 4) == ERR_ARG
    assert lib.vp8drv_set_source_window(drv.h, None, 0, 0) == 0
    assert arf(drv) == 0                                           # ... and with all of them off again it is coded
    assert len(drv.get_frame()) > 3
    assert lib.vp8drv_get_arf_stats(drv.h, C.byref(st)) == 0 and st.hidden_frames == 1
    # a member of a live batch; and a driver with hidden frames on makes no batch
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch([drv])
    drv.close()
    a, b = api.NativeDriver(w, h), api.NativeDriver(w, h)
    batch = api.NativeBatch([a, b])
    assert lib.vp8drv_set_arf(a.h, 4) == ERR_STATE
    batch.close()
    a.close()
    b.close()
    for cfg in (dict(device_params=0), dict(overlap_filter=1)):
        d = api.NativeDriver(w, h, **cfg)
        assert lib.vp8drv_set_arf(d.h, 4) == ERR_ARG, cfg
        assert lib.vp8drv_set_arf(d.h, 0) == 0
        d.close()
    # the context: the same refusals, and the filter beside the next frame as a state (the split and the batch member: the next test)
    hip = api.Vp8Hip(w, h)
    lib.vp8hip_arf_filter_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.vp8hip_arf_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_loop_filter_hidden.argtypes = [C.c_void_p]
    wgt = (C.c_int32 * 3)()
    assert lib.vp8hip_arf_result(hip.h, wgt) == ERR_STATE
    assert lib.vp8hip_loop_filter_hidden(hip.h) == ERR_STATE       # no reconstruction
    for n, centre, s in ((0, 0, 3), (8, 0, 3), (3, 3, 3), (3, 1, 7), (3, 1, -1)):
        assert lib.vp8hip_arf_filter_host(hip.h, table, n, centre, s) == ERR_ARG
    hip.set_denoise(1)
    assert lib.vp8hip_arf_filter_host(hip.h, table, 3, 1, 3) == ERR_ARG
    hip.set_denoise(0)
    hip.filter_overlap(True)
    assert lib.vp8hip_arf_filter_host(hip.h, table, 3, 1, 3) == ERR_STATE
    hip.filter_overlap(False)
    assert lib.vp8hip_arf_filter_host(hip.h, table, 3, 1, 3) == 0
    hip.close()


def test_a_by_reference_split_and_a_batch_member_are_refused_at_both_layers():
    """a context that shares a frame's searches with other devices (vp8hip_shard_init; one rank is enough to make it one) and a context
    that is a member of a live batch: VP8HIP_ERR_STATE from both forms of the filter and from the hidden end, at the context and through
    the driver (which has no check of its own for the split and relies on the context's), and nothing has changed"""
    from vp8oclenc_amd import api, ref_shard
    w, h = 64, 48
    frames = ref.noisy_pan(w, h, 3, seed=2)
    lib = api.load_library()
    for fn in (lib.vp8hip_arf_filter_host, lib.vp8hip_arf_filter_device):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    for fn in (lib.vp8drv_encode_arf_host, lib.vp8drv_encode_arf_device):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.vp8hip_arf_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_loop_filter_hidden.argtypes = [C.c_void_p]
    lib.vp8drv_get_arf_stats.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_shard_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    keep, table = api._plane_table(frames)
    dev = [[api.to_device(p) for p in f] for f in frames]
    dtable = (C.c_void_p * 9)(*[b.data_ptr() for f in dev for b in f])
    wgt, st = (C.c_int32 * 3)(), api.ArfStats()

    def refused(hip):
        before = current_surfaces(hip)
        assert lib.vp8hip_arf_filter_host(hip.h, table, 3, 1, 3) == ERR_STATE
        assert lib.vp8hip_arf_filter_device(hip.h, dtable, 3, 1, 3) == ERR_STATE
        assert lib.vp8hip_arf_result(hip.h, wgt) == ERR_STATE      # no launch, no staging buffer
        same(current_surfaces(hip), before, "the current frame after a refusal")

    # the split, at the context ...
    be = ref_shard.HipRefBackend(w, h)
    be.upload_current(*frames[0])
    be.shard_init(ref_shard.shard_unique_id(), 0, 1)
    refused(be)
    assert lib.vp8hip_loop_filter_hidden(be.h) == ERR_STATE
    be.close()
    # ... and through the driver: a reference exists, hidden frames are on, the context joins a split
    drv = api.NativeDriver(w, h)
    drv.set_arf(4)
    drv.encode_frame_host(*frames[0])
    first = drv.get_frame()
    last = [p.copy() for p in drv.hip.download_last()]
    assert lib.vp8hip_shard_init(drv.hip.h, ref_shard.shard_unique_id(), 0, 1) == 0
    assert lib.vp8drv_encode_arf_host(drv.h, table, 3, 1) == ERR_STATE
    assert lib.vp8drv_encode_arf_device(drv.h, dtable, 3, 1) == ERR_STATE
    assert lib.vp8drv_get_arf_stats(drv.h, C.byref(st)) == ERR_STATE      # none coded
    same(drv.hip.download_last(), last, "LAST after the refusals")
    assert drv.stats().frame_number == 1 and len(first) > 10
    drv.close()
    # a member of a live batch, at the context (the driver's own refusal: test_every_refusal)
    ctxs = [api.Vp8Hip(w, h), api.Vp8Hip(w, h)]
    for c in ctxs:
        c.upload_current(*frames[0])
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    hb = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * 2)(ctxs[0].h, ctxs[1].h), 2) == 0
    for c in ctxs:
        refused(c)
        assert lib.vp8hip_loop_filter_hidden(c.h) == ERR_STATE
    lib.vp8hip_batch_destroy(hb)
    assert lib.vp8hip_arf_filter_host(ctxs[0].h, table, 3, 1, 3) == 0      # on its own again it filters
    for c in ctxs:
        c.close()
    for f in dev:
        for b in f:
            b.free()


def test_a_staged_frame_and_an_armed_check_are_refused():
    """a frame handed over early is the context's current frame and a hidden frame would take its place; a hidden frame has no
    check_SSIM, so its end refuses a reconstruction whose check is armed (the ordinary end then still works)"""
    from vp8oclenc_amd import api
    w, h = 64, 48
    frames = ref.noisy_pan(w, h, 3, seed=3)
    lib = api.load_library()
    lib.vp8drv_encode_arf_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.vp8drv_stage_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vp8hip_loop_filter_hidden.argtypes = [C.c_void_p]
    keep, table = api._plane_table(frames)
    ny, nc = w * h, (w // 2) * (h // 2)
    hb = api.HostBuffer(np.concatenate([p.ravel() for p in frames[1]]))
    ptrs = (hb.data_ptr(), hb.data_ptr() + ny, hb.data_ptr() + ny + nc)
    drv = api.NativeDriver(w, h)
    drv.set_arf(4)
    drv.encode_frame_host(*frames[0])
    drv.get_frame()
    assert lib.vp8drv_stage_frame_host(drv.h, *ptrs) == 0
    assert lib.vp8drv_encode_arf_host(drv.h, table, 3, 1) == ERR_STATE
    plain = api.NativeDriver(w, h)      # the staged frame is still coded as the frame it is
    plain.encode_frame_host(*frames[0])
    plain.get_frame()
    drv.encode_frame_host_ptr(*ptrs)
    plain.encode_frame_host(*frames[1])
    assert drv.get_frame() == plain.get_frame()
    assert lib.vp8drv_encode_arf_host(drv.h, table, 3, 1) == 0      # nothing staged any more
    drv.close()
    plain.close()
    hb.free()
    hip = api.Vp8Hip(w, h)
    refqi, _ = api.quantizer_ladders(0, 48)
    hip.upload_current(*frames[0])
    hip.auto_segments(True, refqi, 0)
    hip.intra_transform()
    hip.prepare_filter_mask(want_nz=False)
    hip.loop_filter()
    assert lib.vp8hip_loop_filter_hidden(hip.h) == ERR_STATE       # the reconstruction has been filtered: there is none
    hip.upload_current(*frames[1])
    hip.auto_segments(False, refqi, 0)
    hip.inter_transform(1, 1, 0, 0)
    hip.check_ssim_async(refqi, 0)
    assert lib.vp8hip_loop_filter_hidden(hip.h) == ERR_STATE       # armed
    hip.loop_filter()                                              # the ordinary end carries the verdict
    assert hip.check_ssim_result()[0] == 0
    hip.close()


def test_scene_detection_sees_the_shown_frames_only():
    """cfg.scene_detect compares every frame taken in with the one before it; a hidden frame steps out of the intake when it is coded, so a
    driver with hidden frames makes key frames of exactly the shown frames a driver without them does (a cut in the middle, and hidden
    frames right in front of it, right behind it and elsewhere), and numbers its quality records alike"""
    from vp8oclenc_amd import api
    w, h = 64, 48
    a = ref.noisy_pan(w, h, 6, seed=4, amplitude=1)
    b = [(y, 255 - u, 255 - v) for y, u, v in ref.noisy_pan(w, h, 6, seed=5, amplitude=1)]      # another picture in other colours: a cut at frame 6
    frames = a + b
    hidden_before = {2: (0, 5, 2), 6: (4, 5, 2), 7: (6, 4, 1), 10: (8, 4, 2)}      # t: (window start, frames, centre) in front of shown frame t
    keys, stats, numbers = [], [], []
    for on in (False, True):
        drv = api.NativeDriver(w, h, gop_size=150, scene_detect=1, quality_stats=1, **QI)
        if on:
            drv.set_arf(4)
        k, qn = [], []
        for t, f in enumerate(frames):
            if on and t in hidden_before:
                lo, n, c = hidden_before[t]
                drv.encode_arf_host(frames[lo:lo + n], c)
                assert not drv.get_frame()[0] & 0x10
            was_key = drv.encode_frame_host(*f)
            drv.get_frame()
            k.append(bool(drv.resolve() or was_key))
            qn.append(int(drv.frame_quality().frame_number))
        keys.append(k)
        numbers.append(qn)
        stats.append(drv.stats().scene_changes)
        drv.close()
    assert keys[0] == keys[1] and stats[0] == stats[1] >= 1 and keys[0][0] and keys[0][6], (keys, stats)
    assert numbers[0] == numbers[1] == list(range(len(frames)))


# ---- 6. off is off ----------------------------------------------------------------------------------------------------------------------------
def test_off_by_default_the_committed_sequence_keeps_its_bytes():
    """a driver that never calls the new entry points, and one that calls vp8drv_set_arf(0), on the small sequence whose digests are
    committed (tests/golden/full_length/selftest.json): every frame's bytes and every reconstruction"""
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
            d.set_arf(0)
        for t in range(doc["frames"]):
            d.encode_frame_host(*source[t % flo.ND])
            b = d.get_frame()
            d.resolve()
            assert (zlib.crc32(b), len(b)) == (doc["frame_crc32"][t], doc["frame_len"][t]), (call, t)
            assert flo.crc_planes(d.hip.download_last()) == doc["recon_crc32"][t], (call, t)
        d.close()


def test_turning_hidden_frames_off_after_use_keeps_the_references():
    """vp8drv_set_arf(0) between a hidden frame and the frames that use it frees the staging buffers only: the stream goes on as the
    oracle loop's does, and turning it on again makes the buffers again"""
    w, h, total, gop = 64, 48, 10, 10
    placement = {0: (0, 4, 3, "after"), 6: (4, 5, 2, "before")}
    frames, recs = oracle_records(w, h, total, gop, tuple(sorted(placement.items())), 3, 0, altref_range=20)
    seen = run_driver(frames, recs, 1, stop_after=1, gop_size=gop, altref_range=20, ref_mask=3, **QI)
    assert seen["hidden"] == 2
