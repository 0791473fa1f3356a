"""Interlaced source frames made progressive on the device (vp8hip_set_deinterlace, k_deinterlace_b): the kernel against the numpy
restatement of tests/deinterlace_ref.py byte for byte whichever way a frame comes in, behind a format converter, and composed with
everything downstream -- a driver that deinterlaces is a driver fed the restatement's frames (restarted where the GOP schedule starts a
GOP), alone and in a batch.  Everything is exact: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import deinterlace_ref as ref

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


def take(hip, frame, way):
    from vp8oclenc_amd import api
    if way == "device":
        d = [api.to_device(p) for p in frame]
        hip.set_current_device(*[b.data_ptr() for b in d])
        hip.synchronize()
    else:
        hip.upload_current(*frame)


def record(r):
    return (r.frame_number, r.woven, r.missing)


# (coded size, source size or None, incoming size of a scaler or None).  16x16: chroma narrower than a strip of 16; 48x32: whole strips and a
# chroma row of one and a half; 56x40 and 50x36 in 64x48: last strips moved left, rows that start at odd bytes (chroma 25 wide), padding
# behind; 128x96 scaled to 64x48: the scaler reads the deinterlacer's output
SHAPES = [((16, 16), None, None), ((48, 32), None, None), ((64, 48), (56, 40), None), ((64, 48), (50, 36), None), ((64, 48), None, (128, 96))]


# ---- 1. the context: kernel against restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["device", "upload"])
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("coded,src,scaled", SHAPES)
def test_kernel_equals_the_restatement_byte_for_byte(coded, src, scaled, mode, keep, way):
    from vp8oclenc_amd import api
    W, H = coded
    iw, ih = scaled or src or coded
    plain, di = api.Vp8Hip(W, H), api.Vp8Hip(W, H)      # `plain` pads / scales the restatement's frames: what the pack is given
    for hip in (plain, di):
        if scaled:
            hip.set_source_scaling(iw, ih, W, H, api.SCALE_AREA)
        elif src:
            hip.set_source_size(*src)
    di.set_deinterlace(mode, keep)
    seqs = ref.sequences(iw, ih, seed=7 + 2 * mode + keep)
    for name in ("moving", "static", "half_static"):
        d = ref.Deinterlacer(mode, keep)
        di.deinterlace_restart()
        woven = []
        for t, f in enumerate(seqs[name]):
            want, n, missing = d.take(f)
            take(plain, want, way)
            take(di, f, way)
            assert_surfaces(current_surfaces(di), current_surfaces(plain), f"{name} frame {t}")
            r = di.deinterlace_result()
            assert (r.woven, r.missing) == (n, missing) and missing == iw * ih // 2, (name, t)
            woven.append(n)
        if mode == 2:
            assert woven[0] == 0
            if name == "half_static":
                assert all(n > 0 for n in woven[1:])
            if name == "static":
                assert all(n == iw * ih // 2 for n in woven[1:])
        else:
            assert not any(woven)
    assert di.deinterlace_result().frame_number == 14      # the 15th frame this context took in
    plain.close()
    di.close()


# ---- 2. behind a format converter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "yuy2"])
def test_chain_with_a_converter(fmt):
    from vp8oclenc_amd import api
    import packed_format_ref as P
    (W, H), (w, h) = (64, 48), (56, 40)
    plain, di = api.Vp8Hip(W, H), api.Vp8Hip(W, H)
    for hip in (plain, di):
        hip.set_source_size(w, h)
    di.set_source_format(fmt)
    di.set_deinterlace(2, 1)
    d = ref.Deinterlacer(2, 1)
    rng = np.random.default_rng(31)
    for t, f in enumerate(ref.sequences(w, h, seed=13)["half_static"]):
        if fmt == "nv12":
            planes = api.planes_from_i420(api.FORMAT_NV12, *f)
            planes, i420 = [planes[0], planes[1], planes[1]], f
        else:      # 4:2:2 chroma of its own: the converter's vertical average is in the chain
            c = [np.repeat(p, 2, axis=0) for p in f[1:]]
            if t:
                c = [np.clip(p.astype(int) + rng.integers(-9, 10, p.shape) * (np.arange(p.shape[1]) >= p.shape[1] // 2), 0, 255) for p in c]
            packed = P.make_422(P.YUY2, f[0], *c)
            planes, i420 = [packed] * 3, P.convert_ref(P.YUY2, w, h, packed)
        want, n, missing = d.take(i420)
        plain.upload_current(*want)
        if t & 1:
            dev = [api.to_device(p) for p in planes]
            di.set_current_device(*[b.data_ptr() for b in dev])
            di.synchronize()
        else:
            di.upload_current(*planes)
        assert_surfaces(current_surfaces(di), current_surfaces(plain), f"{fmt} frame {t}")
        assert record(di.deinterlace_result()) == (t, n, missing)
        assert t == 0 or n > 0
    plain.close()
    di.close()


# ---- 3. the setting changes ----------------------------------------------------------------------------------------------------------
def test_setting_changes_and_restart():
    from vp8oclenc_amd import api
    W, H = 48, 32
    hip = api.Vp8Hip(W, H)
    frames = ref.sequences(W, H, seed=9)["half_static"] + ref.sequences(W, H, seed=10)["half_static"] + ref.sequences(W, H, seed=11)["half_static"]
    lib = hip.lib
    lib.vp8hip_deinterlace_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_set_deinterlace.argtypes = [C.c_void_p, C.c_int, C.c_int]
    s = api.DeinterlaceStats()
    assert lib.vp8hip_deinterlace_result(hip.h, C.byref(s)) == ERR_STATE      # off
    hip.set_deinterlace(2, 0)
    assert lib.vp8hip_deinterlace_result(hip.h, C.byref(s)) == ERR_STATE      # on, nothing taken in
    d = ref.Deinterlacer(2, 0)
    for f in frames[:3]:
        hip.upload_current(*f)
        assert_surfaces(current_surfaces(hip), d.take(f)[0], "adaptive, top")
    for bad in ((3, 0), (-1, 0), (2, 2), (1, -1)):
        assert lib.vp8hip_set_deinterlace(hip.h, *bad) == ERR_ARG
    hip.upload_current(*frames[3])      # a refused argument changed nothing: the same mode, parity and history
    want, n, _ = d.take(frames[3])
    assert_surfaces(current_surfaces(hip), want, "after refusals")
    assert hip.deinterlace_result().woven == n > 0
    hip.set_deinterlace(2, 0)           # the same setting again: nothing restarts
    hip.upload_current(*frames[4])
    want, n, _ = d.take(frames[4])
    assert_surfaces(current_surfaces(hip), want, "same setting")
    assert hip.deinterlace_result().woven == n > 0
    hip.deinterlace_restart()
    d.restart()
    hip.upload_current(*frames[5])
    want, n, _ = d.take(frames[5])
    assert n == 0
    assert_surfaces(current_surfaces(hip), want, "restart")
    assert_surfaces(current_surfaces(hip), ref.Deinterlacer(1, 0).take(frames[5])[0], "a frame without a history is mode 1's")
    hip.set_deinterlace(0, 0)           # off: pass-through again
    hip.upload_current(*frames[6])
    assert_surfaces(current_surfaces(hip), frames[6], "off")
    assert lib.vp8hip_deinterlace_result(hip.h, C.byref(s)) == ERR_STATE
    for mode, keep in ((2, 1), (1, 1), (2, 1), (2, 0)):      # on from off, a mode change, back, a parity change: a new history each time
        hip.set_deinterlace(mode, keep)
        d = ref.Deinterlacer(mode, keep)
        for t, f in enumerate(frames[7:10]):
            hip.upload_current(*f)
            want, n, missing = d.take(f)
            assert_surfaces(current_surfaces(hip), want, f"mode {mode} keep {keep} frame {t}")
            r = hip.deinterlace_result()
            assert (r.woven, r.missing) == (n, missing)
            assert (n > 0) == (mode == 2 and t > 0)
    hip.close()


def test_errors():
    from vp8oclenc_amd import api
    drv = api.NativeDriver(64, 48)
    lib = drv.lib
    lib.vp8drv_set_deinterlace.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8drv_get_deinterlace_stats.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_set_deinterlace.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8hip_deinterlace_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_set_source_size.argtypes = [C.c_void_p, C.c_int, C.c_int]
    s = api.DeinterlaceStats()
    for bad in ((3, 0), (-1, 0), (1, 2), (2, -1)):
        assert lib.vp8drv_set_deinterlace(drv.h, *bad) == ERR_ARG
    assert lib.vp8drv_get_deinterlace_stats(drv.h, C.byref(s)) == ERR_STATE
    assert lib.vp8drv_set_deinterlace(drv.h, 2, 1) == 0
    assert lib.vp8drv_get_deinterlace_stats(drv.h, C.byref(s)) == ERR_STATE      # nothing taken in yet
    assert lib.vp8drv_get_deinterlace_stats(drv.h, None) == ERR_ARG
    drv.close()
    mirror = api.NativeDriver(64, 48, device_params=0)
    assert lib.vp8drv_set_deinterlace(mirror.h, 2, 0) == ERR_ARG                   # the host mirror would scan the caller's luma
    mirror.close()
    hip = api.Vp8Hip(16, 16)
    assert lib.vp8hip_set_deinterlace(hip.h, 3, 0) == ERR_ARG
    assert lib.vp8hip_deinterlace_result(hip.h, C.byref(s)) == ERR_STATE
    assert lib.vp8hip_deinterlace_result(hip.h, None) == ERR_ARG
    hip.set_source_size(16, 2)
    assert lib.vp8hip_set_deinterlace(hip.h, 1, 0) == ERR_ARG                      # height 2: the chroma planes have one row
    hip.set_source_size(16, 4)
    assert lib.vp8hip_set_deinterlace(hip.h, 1, 0) == 0
    assert lib.vp8hip_set_source_size(hip.h, 16, 2) == ERR_ARG                     # ... whichever setter comes second
    f = ref.sequences(16, 4, seed=2)["moving"][0]
    hip.upload_current(*f)                                                         # (and the size that was refused is not in force)
    plain = api.Vp8Hip(16, 16)
    plain.set_source_size(16, 4)
    plain.upload_current(*ref.Deinterlacer(1, 0).take(f)[0])
    assert_surfaces(current_surfaces(hip), current_surfaces(plain), "16x4")
    plain.close()
    hip.close()


# ---- 4. the driver, end to end ------------------------------------------------------------------------------------------------------
DRV_CFG = dict(gop_size=4, altref_range=2, check_ssim=1, ref_mask=3, num_partitions=2, quality_stats=1)


class Schedule:
    """the driver's GOP schedule mirrored: which incoming frames it makes key frames, given how the frames before ended"""

    def __init__(self, cfg):
        from vp8oclenc_amd import api
        self.g = api.Gop(cfg["gop_size"], cfg["altref_range"])

    def incoming_is_key(self):
        return bool(self.g.next().current_is_key)

    def done(self, ended_as_key):
        if ended_as_key:
            self.g.key_coded()
        self.g.frame_done()


def run_pair(frames, way, ssim_target, mode=2, keep=0, **more):
    """driver `a` deinterlaces on the device, driver `b` is fed the restatement's frames -> (a's statistics, frames the schedule
    restarted at, woven counts)"""
    from vp8oclenc_amd import api
    W, H = frames[0][0].shape[1], frames[0][0].shape[0]
    cfg = dict(DRV_CFG, ssim_target=ssim_target, **more)
    a, b = api.NativeDriver(W, H, **cfg), api.NativeDriver(W, H, **cfg)
    a.set_deinterlace(mode, keep)
    d, sched = ref.Deinterlacer(mode, keep), Schedule(cfg)
    ny, nc = W * H, (W // 2) * (H // 2)
    host = [api.HostBuffer(np.concatenate([p.ravel() for p in f])) for f in frames]
    ptrs = [(hb.data_ptr(), hb.data_ptr() + ny, hb.data_ptr() + ny + nc) for hb in host]
    a.lib.vp8drv_stage_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    restarts, counts = [], []
    for t, f in enumerate(frames):
        if sched.incoming_is_key():
            d.restart()
            restarts.append(t)
        clean, n, missing = d.take(f)
        if way == "device":
            dev = [api.to_device(p) for p in f]
            a.encode_frame_device(*[x.data_ptr() for x in dev])
        elif way == "host":
            a.encode_frame_host(*f)
        elif way == "prefetch":
            if t == 0:
                a.prefetch_frame_host_ptr(*ptrs[0])
            a.encode_frame_host_ptr(*ptrs[t])
            if t + 1 < len(frames):
                a.prefetch_frame_host_ptr(*ptrs[t + 1])
        else:      # stage: frame t was handed over early behind frame t - 1, below
            a.encode_frame_host_ptr(*ptrs[t])
        b.encode_frame_host(*clean)
        assert record(a.deinterlace_stats()) == (t, n, missing), t
        counts.append(n)
        fa, fb = a.get_frame(), b.get_frame()
        assert fa == fb, f"{way}: frame {t}: {len(fa)} vs {len(fb)} bytes"
        assert bytes(a.frame_quality()) == bytes(b.frame_quality()), (way, t)
        for p, q in zip(a.hip.download_last(), b.hip.download_last()):
            assert np.array_equal(p, q), (way, t)
        ended_key = a.resolve()
        assert ended_key == (not (fa[0] & 1)) == b.resolve()
        sched.done(ended_key)
        if way == "stage" and t + 1 < len(frames):
            assert a.lib.vp8drv_stage_frame_host(a.h, *ptrs[t + 1]) == 0
    assert bytes(a.quality_summary()) == bytes(b.quality_summary())
    stats = a.stats()
    a.close()
    b.close()
    for hb in host:
        hb.free()
    return stats, restarts, counts


@pytest.mark.parametrize("way", ["device", "host", "prefetch", "stage"])
def test_a_driver_that_deinterlaces_equals_a_driver_fed_the_restatements_frames(way):
    frames = ref.interlaced_video(64, 48, 8, seed=3)
    stats, restarts, counts = run_pair(frames, way, ssim_target=-1.0)
    assert restarts == [0, 4] and stats.redone_as_key == 0
    assert counts[0] == counts[4] == 0 and all(c > 0 for i, c in enumerate(counts) if i not in (0, 4))


def test_a_frame_sent_back_by_check_ssim_is_not_deinterlaced_twice():
    # a cut at frame 2: check_SSIM sends the frame back, it is coded again as a key frame from the SAME current frame (deinterlaced once:
    # the stream equals the driver's that was fed the restatement's frames), and the history does not restart there
    # (fresh noise below the rows that stand still: a clean picture codes above the target even across the cut)
    frames = ref.interlaced_video(64, 48, 8, seed=4, cut_at=2, keep=1, noise=4)
    # (coarse quantizers and a target of 0.95: the inter version of the cut frame falls below it)
    stats, restarts, counts = run_pair(frames, "device", ssim_target=0.95, keep=1, qi_min=50, qi_max=110)
    print("redone_as_key", stats.redone_as_key, "restarts", restarts, "woven", counts)
    assert stats.redone_as_key >= 1
    assert restarts[0] == 0 and 2 not in restarts and 3 not in restarts
    assert counts[2] > 0 and counts[3] > 0      # the frames behind frames that were sent back find them, as received, as their history


# ---- 5. batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_a_batch_of_two_equals_the_two_alone(host):
    from vp8oclenc_amd import api
    W, H, steps = 64, 48, 6
    seqs = [ref.interlaced_video(W, H, steps, seed=20 + i) for i in range(2)]
    cfg = dict(gop_size=3, num_partitions=2)
    alone = []
    for i in range(2):
        drv = api.NativeDriver(W, H, **cfg)
        drv.set_deinterlace(2, 0)
        out = []
        for f in seqs[i]:
            drv.encode_frame_host(*f)
            out.append((drv.get_frame(), record(drv.deinterlace_stats())))
        drv.close()
        alone.append(out)
    assert any(r[1] > 0 for _, r in alone[0]) and alone[0] != alone[1]
    drvs = [api.NativeDriver(W, H, **cfg) for _ in range(2)]
    for d in drvs:
        d.set_deinterlace(2, 0)
    batch = api.NativeBatch(drvs)
    drvs[0].lib.vp8drv_set_deinterlace.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert drvs[0].lib.vp8drv_set_deinterlace(drvs[0].h, 1, 0) == ERR_STATE      # a member of a live batch
    ny, nc = W * H, (W // 2) * (H // 2)
    for t in range(steps):
        if host:
            bufs = [api.HostBuffer(np.concatenate([p.ravel() for p in s[t]])) for s in seqs]
        else:
            bufs = [api.to_device(np.concatenate([p.ravel() for p in s[t]])) for s in seqs]
        batch.encode_frame_device([(b.data_ptr(), b.data_ptr() + ny, b.data_ptr() + ny + nc) for b in bufs], host=host)
        for i, d in enumerate(drvs):
            assert (d.get_frame(), record(d.deinterlace_stats())) == alone[i][t], (t, i)
        for b in bufs:
            b.free()
    batch.close()
    for d in drvs:
        d.close()


@pytest.mark.parametrize("a,b", [((2, 0), (1, 0)), ((2, 0), (2, 1)), ((1, 1), (0, 0))])
def test_members_that_differ_in_mode_or_parity_make_no_batch(a, b):
    from vp8oclenc_amd import api
    W, H = 64, 48
    odd = [api.NativeDriver(W, H, gop_size=3), api.NativeDriver(W, H, gop_size=3)]
    odd[0].set_deinterlace(*a)
    odd[1].set_deinterlace(*b)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(odd)
    for d in odd:
        d.close()
    ctxs = [api.Vp8Hip(W, H), api.Vp8Hip(W, H)]
    ctxs[0].set_deinterlace(*a)
    ctxs[1].set_deinterlace(*b)
    lib = ctxs[0].lib
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    h = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(h), (C.c_void_p * 2)(ctxs[0].h, ctxs[1].h), 2) == ERR_ARG
    for c in ctxs:
        c.close()


def test_a_member_whose_deinterlacer_was_on_and_is_off_again_batches_with_one_that_never_had_it():
    """off is off whatever parity the call that turned it off named: set_deinterlace(1, 0) and then (0, 1) leaves nothing behind"""
    from vp8oclenc_amd import api
    W, H = 64, 48
    ctxs, alone = [api.Vp8Hip(W, H), api.Vp8Hip(W, H)], [api.Vp8Hip(W, H), api.Vp8Hip(W, H)]
    for group in (ctxs, alone):
        group[0].set_deinterlace(1, 0)
        group[0].set_deinterlace(0, 1)
    lib = ctxs[0].lib
    arr = C.POINTER(C.c_void_p)
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), arr, C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
    lib.vp8hip_batch_destroy.restype = None
    lib.vp8hip_batch_upload_current.argtypes = [C.c_void_p, C.POINTER(C.c_int), arr, arr, arr]
    hb = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * 2)(ctxs[0].h, ctxs[1].h), 2) == 0
    videos = [ref.interlaced_video(W, H, 2, seed=51), ref.interlaced_video(W, H, 2, seed=52)]
    for t in range(2):
        bufs = [[api.HostBuffer(p) for p in v[t]] for v in videos]
        planes = [(C.c_void_p * 2)(bufs[0][k].data_ptr(), bufs[1][k].data_ptr()) for k in range(3)]
        assert lib.vp8hip_batch_upload_current(hb, None, *planes) == 0
        for i in range(2):
            ctxs[i].synchronize()
            alone[i].upload_current(*videos[i][t])
            assert_surfaces(current_surfaces(ctxs[i]), current_surfaces(alone[i]), f"member {i} frame {t}")
            assert_surfaces(current_surfaces(ctxs[i]), videos[i][t], f"member {i} frame {t}: passed through")
        for v in bufs:
            for b in v:
                b.free()
    lib.vp8hip_batch_destroy(hb)
    for c in ctxs + alone:
        c.close()


# ---- 6. beside the denoiser and the analysis ------------------------------------------------------------------------------------------
def test_the_order_is_deinterlace_then_denoise_then_analysis():
    from vp8oclenc_amd import api
    import analysis_ref
    import denoise_ref
    W, H = 64, 48
    hip = api.Vp8Hip(W, H)
    hip.set_analysis(True)      # (the setters in another order than the stages)
    hip.set_denoise(2)
    hip.set_deinterlace(2, 0)
    di, dn = ref.Deinterlacer(2, 0), denoise_ref.Denoiser(2)
    prev, filtered, woven = None, 0, 0
    fields = analysis_ref.SOURCE_FIELDS
    for t, f in enumerate(ref.interlaced_video(W, H, 5, seed=41)):
        hip.upload_current(*f)
        progressive, n, missing = di.take(f)
        clean, m, _ = dn.take(progressive)
        assert_surfaces(current_surfaces(hip), clean, f"frame {t}")
        assert record(hip.deinterlace_result()) == (t, n, missing) and hip.denoise_result().mbs_filtered == m
        rec, want = hip.analysis_result(), analysis_ref.source_side(clean[0], prev)
        assert {k: int(getattr(rec, k)) for k in fields} == want, t
        prev = clean[0]
        filtered += m
        woven += n
    assert filtered > 0 and woven > 0      # (both stages did something: the order is what was tested)
    hip.close()


# ---- 7. off is off ---------------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    from vp8oclenc_amd import api
    frames = ref.interlaced_video(64, 48, 8, seed=3)
    cfg = dict(DRV_CFG, ssim_target=-1.0)
    outs = []
    for call in (False, True):
        drv = api.NativeDriver(64, 48, **cfg)
        if call:
            drv.set_deinterlace(0, 0)
        out = []
        for f in frames:
            drv.encode_frame_host(*f)
            out.append(drv.get_frame())
            out.append(bytes(drv.frame_quality()))
        drv.close()
        outs.append(out)
    assert outs[0] == outs[1]
    on = api.NativeDriver(64, 48, **cfg)
    on.set_deinterlace(2, 0)
    changed = False
    for t, f in enumerate(frames):
        on.encode_frame_host(*f)
        changed |= on.get_frame() != outs[0][2 * t]
    on.close()
    assert changed      # (and on is on)
