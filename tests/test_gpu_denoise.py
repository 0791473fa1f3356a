"""Temporal noise reduction of the source frames on the device (vp8hip_set_denoise, k_denoise_b): the kernel against the numpy
restatement of tests/denoise_ref.py byte for byte whichever way a frame comes in, and composed with everything downstream -- a driver
that denoises is a driver fed the restatement's frames (restarted where the GOP schedule starts a GOP), alone and in a batch.
Everything is exact: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as ref

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


# (coded size, source size or None, incoming size of a scaler or None)
SHAPES = [((16, 16), None, None), ((48, 32), None, None), ((64, 48), (56, 40), None), ((64, 48), None, (128, 96))]


# ---- 1. the context: kernel against restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["device", "upload"])
@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("coded,src,scaled", SHAPES)
def test_kernel_equals_the_restatement_byte_for_byte(coded, src, scaled, level, way):
    from vp8oclenc_amd import api
    W, H = coded
    iw, ih = scaled or src or coded
    plain, dn = api.Vp8Hip(W, H), api.Vp8Hip(W, H)      # `plain` packs / pads / scales the same frames: what the denoiser is given
    for hip in (plain, dn):
        if scaled:
            hip.set_source_scaling(iw, ih, W, H, api.SCALE_AREA)
        elif src:
            hip.set_source_size(*src)
    dn.set_denoise(level)
    seqs = ref.sequences(iw, ih, seed=5 + level)
    for name in ("wild", "mixed", "moving_stripe"):
        d = ref.Denoiser(level)
        dn.denoise_restart()
        for t, f in enumerate(seqs[name]):
            take(plain, f, way)
            take(dn, f, way)
            packed = current_surfaces(plain)
            assert packed[0].shape == (H, W)
            want, n, _ = d.take(packed)
            assert_surfaces(current_surfaces(dn), want, f"{name} frame {t}")
            r = dn.denoise_result()
            assert (r.mbs_filtered, r.mbs_total) == (n, (W // 16) * (H // 16)), (name, t)
        if name == "wild" and W > 16:
            assert 0 < n      # (something was filtered: the test is not about pass-through)
    r = dn.denoise_result()
    assert r.frame_number == 14      # the 15th frame this context took in
    plain.close()
    dn.close()


def test_off_after_on_and_a_level_change():
    from vp8oclenc_amd import api
    W, H = 48, 32
    hip = api.Vp8Hip(W, H)
    frames = ref.sequences(W, H, seed=9)["wild"] + ref.sequences(W, H, seed=10)["static_noise"]
    lib = hip.lib
    lib.vp8hip_denoise_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_set_denoise.argtypes = [C.c_void_p, C.c_int]
    s = api.DenoiseStats()
    assert lib.vp8hip_denoise_result(hip.h, C.byref(s)) == ERR_STATE      # off
    hip.set_denoise(2)
    assert lib.vp8hip_denoise_result(hip.h, C.byref(s)) == ERR_STATE      # on, nothing taken in
    d = ref.Denoiser(2)
    for f in frames[:3]:
        hip.upload_current(*f)
        assert_surfaces(current_surfaces(hip), d.take(f)[0], "level 2")
    for bad in (4, -1):
        assert lib.vp8hip_set_denoise(hip.h, bad) == ERR_ARG
    hip.upload_current(*frames[3])      # a refused level changed nothing: still level 2, still the same history
    d2 = ref.Denoiser(2)
    for f in frames[:4]:
        want = d2.take(f)[0]
    assert_surfaces(current_surfaces(hip), want, "after refusals")
    hip.set_denoise(0)                   # off: pass-through again
    hip.upload_current(*frames[4])
    assert_surfaces(current_surfaces(hip), frames[4], "off")
    assert lib.vp8hip_denoise_result(hip.h, C.byref(s)) == ERR_STATE
    hip.set_denoise(1)                   # on from off: a new history
    d = ref.Denoiser(1)
    for t, f in enumerate(frames[5:8]):
        hip.upload_current(*f)
        want, n, _ = d.take(f)
        assert_surfaces(current_surfaces(hip), want, f"level 1 frame {t}")
        assert hip.denoise_result().mbs_filtered == n
        if t == 0:
            assert_surfaces(current_surfaces(hip), f, "the first frame passes through")
    hip.set_denoise(3)                   # a level change restarts the history
    d = ref.Denoiser(3)
    for t, f in enumerate(frames[8:]):
        hip.upload_current(*f)
        assert_surfaces(current_surfaces(hip), d.take(f)[0], f"level 3 frame {t}")
        if t == 0:
            assert_surfaces(current_surfaces(hip), f, "the frame behind a level change passes through")
    hip.set_denoise(3)                   # the same level again: nothing restarts
    hip.upload_current(*frames[0])
    assert_surfaces(current_surfaces(hip), d.take(frames[0])[0], "same level")
    hip.close()


# ---- 2. the driver, end to end ------------------------------------------------------------------------------------------------------
def noisy_video(w, h, n, seed, cut_at=None):
    """a picture that drifts one sample per frame under noise of amplitude 4; from cut_at on another picture altogether"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w + n]
    pics = []
    for k in range(2):
        y = 128 + 60 * np.sin((xx + 11 * k) / (5.0 + 4 * k)) * np.cos(yy / (7.0 - 3 * k)) + 25 * (((xx >> 3) + (yy >> 3) + k) & 1)
        pics.append((y, 128 + 30 * np.sin(xx[:h // 2, :] / 9.0 + k), 128 + 30 * np.cos(yy[:h // 2, :] / 6.0 + 2 * k)))
    out = []
    for t in range(n):
        y, u, v = pics[1 if cut_at is not None and t >= cut_at else 0]
        nz = lambda s: rng.integers(-4, 5, s)
        out.append(tuple(np.ascontiguousarray(np.clip(p, 0, 255), dtype=np.uint8) for p in
                         (y[:, t:t + w] + nz((h, w)), u[:, t // 2:t // 2 + w // 2] + nz((h // 2, w // 2)), v[:, t // 2:t // 2 + w // 2] + nz((h // 2, w // 2)))))
    return out


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


def run_pair(frames, way, ssim_target, level=2, **more):
    """driver `a` denoises on the device, driver `b` is fed the restatement's frames -> (streams equal frame by frame, a's statistics,
    frames the schedule restarted at, filtered counts)"""
    from vp8oclenc_amd import api
    W, H = frames[0][0].shape[1], frames[0][0].shape[0]
    cfg = dict(DRV_CFG, ssim_target=ssim_target, **more)
    a, b = api.NativeDriver(W, H, **cfg), api.NativeDriver(W, H, **cfg)
    a.set_denoise(level)
    d, sched = ref.Denoiser(level), Schedule(cfg)
    ny, nc = W * H, (W // 2) * (H // 2)
    host = [api.HostBuffer(np.concatenate([p.ravel() for p in f])) for f in frames]
    ptrs = [(hb.data_ptr(), hb.data_ptr() + ny, hb.data_ptr() + ny + nc) for hb in host]
    a.lib.vp8drv_stage_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    restarts, counts = [], []
    for t, f in enumerate(frames):
        if sched.incoming_is_key():
            d.restart()
            restarts.append(t)
        clean, n, _ = d.take(f)
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
        st = a.denoise_stats()
        assert (st.frame_number, st.mbs_filtered, st.mbs_total) == (t, n, (W // 16) * (H // 16)), t
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
def test_a_driver_that_denoises_equals_a_driver_fed_the_restatements_frames(way):
    frames = noisy_video(64, 48, 8, seed=3)
    stats, restarts, counts = run_pair(frames, way, ssim_target=-1.0)
    assert restarts == [0, 4] and stats.redone_as_key == 0
    assert counts[0] == counts[4] == 0 and all(c > 0 for i, c in enumerate(counts) if i not in (0, 4))


def test_a_frame_sent_back_by_check_ssim_is_not_denoised_twice():
    # a cut at frame 2: check_SSIM sends the frame back, it is coded again as a key frame from the SAME current frame (denoised once:
    # the stream equals the pre-denoised driver's), and the history does not restart there (the schedule's next restart is the only one)
    frames = noisy_video(64, 48, 8, seed=4, cut_at=2)
    # (coarse quantizers and a target of 0.95: the inter version of the cut frame falls below it)
    stats, restarts, counts = run_pair(frames, "device", ssim_target=0.95, qi_min=50, qi_max=110)
    print("redone_as_key", stats.redone_as_key, "restarts", restarts, "filtered", counts)
    assert stats.redone_as_key >= 1
    assert restarts[0] == 0 and 2 not in restarts and 3 not in restarts
    assert counts[2] == 0 and counts[3] > 0      # the cut is copied by the block decision; the frame behind it finds the cut frame as its history


# ---- 3. batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_a_batch_of_two_equals_the_two_alone(host):
    from vp8oclenc_amd import api
    W, H, steps = 64, 48, 6
    seqs = [noisy_video(W, H, steps, seed=20 + i) for i in range(2)]
    cfg = dict(gop_size=3, num_partitions=2)
    alone = []
    for i in range(2):
        drv = api.NativeDriver(W, H, **cfg)
        drv.set_denoise(2)
        out = []
        for f in seqs[i]:
            drv.encode_frame_host(*f)
            out.append((drv.get_frame(), drv.denoise_stats().mbs_filtered))
        drv.close()
        alone.append(out)
    assert any(n > 0 for _, n in alone[0]) and alone[0] != alone[1]
    drvs = [api.NativeDriver(W, H, **cfg) for _ in range(2)]
    for d in drvs:
        d.set_denoise(2)
    batch = api.NativeBatch(drvs)
    drvs[0].lib.vp8drv_set_denoise.argtypes = [C.c_void_p, C.c_int]
    assert drvs[0].lib.vp8drv_set_denoise(drvs[0].h, 1) == ERR_STATE      # a member of a live batch
    ny, nc = W * H, (W // 2) * (H // 2)
    for t in range(steps):
        if host:
            bufs = [api.HostBuffer(np.concatenate([p.ravel() for p in s[t]])) for s in seqs]
        else:
            bufs = [api.to_device(np.concatenate([p.ravel() for p in s[t]])) for s in seqs]
        batch.encode_frame_device([(b.data_ptr(), b.data_ptr() + ny, b.data_ptr() + ny + nc) for b in bufs], host=host)
        for i, d in enumerate(drvs):
            assert (d.get_frame(), d.denoise_stats().mbs_filtered) == alone[i][t], (t, i)
        for b in bufs:
            b.free()
    batch.close()
    for d in drvs:
        d.close()
    # members that disagree on the level do not make a batch, at either layer
    odd = [api.NativeDriver(W, H, **cfg), api.NativeDriver(W, H, **cfg)]
    odd[1].set_denoise(1)
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch(odd)
    for d in odd:
        d.close()
    ctxs = [api.Vp8Hip(W, H), api.Vp8Hip(W, H)]
    ctxs[0].set_denoise(2)
    ctxs[1].set_denoise(3)
    lib = ctxs[0].lib
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    h = C.c_void_p()
    assert lib.vp8hip_batch_create(C.byref(h), (C.c_void_p * 2)(ctxs[0].h, ctxs[1].h), 2) == ERR_ARG
    for c in ctxs:
        c.close()


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from vp8oclenc_amd import api
    drv = api.NativeDriver(64, 48)
    lib = drv.lib
    lib.vp8drv_set_denoise.argtypes = [C.c_void_p, C.c_int]
    lib.vp8drv_get_denoise_stats.argtypes = [C.c_void_p, C.c_void_p]
    s = api.DenoiseStats()
    assert lib.vp8drv_set_denoise(drv.h, 4) == ERR_ARG and lib.vp8drv_set_denoise(drv.h, -1) == ERR_ARG
    assert lib.vp8drv_get_denoise_stats(drv.h, C.byref(s)) == ERR_STATE
    assert lib.vp8drv_set_denoise(drv.h, 3) == 0
    assert lib.vp8drv_get_denoise_stats(drv.h, C.byref(s)) == ERR_STATE      # nothing taken in yet
    drv.close()
    mirror = api.NativeDriver(64, 48, device_params=0)
    assert lib.vp8drv_set_denoise(mirror.h, 2) == ERR_ARG                      # the host mirror would scan the caller's luma
    mirror.close()
    hip = api.Vp8Hip(64, 48)
    lib.vp8hip_set_denoise.argtypes = [C.c_void_p, C.c_int]
    lib.vp8hip_denoise_result.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.vp8hip_set_denoise(hip.h, 4) == ERR_ARG
    assert lib.vp8hip_denoise_result(hip.h, C.byref(s)) == ERR_STATE
    hip.close()


# ---- 5. off is off ---------------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    from vp8oclenc_amd import api
    frames = noisy_video(64, 48, 8, seed=3)
    cfg = dict(DRV_CFG, ssim_target=-1.0)
    outs = []
    for call in (False, True):
        drv = api.NativeDriver(64, 48, **cfg)
        if call:
            drv.set_denoise(0)
        out = []
        for f in frames:
            drv.encode_frame_host(*f)
            out.append(drv.get_frame())
            out.append(bytes(drv.frame_quality()))
        drv.close()
        outs.append(out)
    assert outs[0] == outs[1]
    on = api.NativeDriver(64, 48, **cfg)
    on.set_denoise(2)
    changed = False
    for t, f in enumerate(frames):
        on.encode_frame_host(*f)
        changed |= on.get_frame() != outs[0][2 * t]
    on.close()
    assert changed      # (and on is on)
