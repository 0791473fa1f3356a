"""PSNR and SSIM of every coded frame, measured on the device (vp8hip_set_quality_stats, vp8drv_config.quality_stats, kernels_quality.hip),
held to the numpy restatement of tests/test_quality_cpu.py on the reconstruction the context hands out and the source as handed in."""
import ctypes as C

import numpy as np
import pytest

from test_quality_cpu import frame_stats, planes
from vp8oclenc_amd import api
from vp8oclenc_amd.synth import SynthSequence

pytestmark = pytest.mark.gpu


def _same(rec, want, what):
    assert list(rec.sse) == want["sse"], (what, list(rec.sse), want["sse"])
    assert list(rec.samples) == want["samples"], what
    assert list(rec.psnr) == pytest.approx(want["psnr"], rel=1e-12) and rec.psnr_all == pytest.approx(want["psnr_all"], rel=1e-12), what
    assert list(rec.ssim) == pytest.approx(want["ssim"], rel=1e-9) and rec.ssim_all == pytest.approx(want["ssim_all"], rel=1e-9), what


def _bits(q):
    return bytes(q)


@pytest.fixture(scope="module")
def hip():
    h = api.Vp8Hip(64, 64)
    yield h
    h.close()


@pytest.mark.parametrize("W,H,kind", [(64, 48, "random"), (17, 9, "random"), (1918, 1078, "random"), (320, 180, "same"),
                                      (3840, 2160, "extreme"), (36, 20, "near")])
def test_the_kernel_on_caller_planes_equals_the_restatement(hip, W, H, kind):
    rng = np.random.default_rng(W * 7 + H)
    if kind == "extreme":      # all 0 against all 255: the squared error needs 64 bits
        src, rec = planes(W, H, lambda s: np.zeros(s, np.uint8)), planes(W, H, lambda s: np.full(s, 255, np.uint8))
    else:
        src = planes(W, H, lambda s: rng.integers(0, 256, s, dtype=np.uint8))
        if kind == "same":
            rec = [p.copy() for p in src]
        elif kind == "near":
            rec = [np.clip(p.astype(int) + rng.integers(-3, 4, p.shape), 0, 255).astype(np.uint8) for p in src]
        else:
            rec = planes(W, H, lambda s: rng.integers(0, 256, s, dtype=np.uint8))
    a = hip.debug_quality(src, rec)
    _same(a, frame_stats(src, rec, W, H), (W, H, kind))
    if kind == "extreme":
        assert a.sse[0] == W * H * 255 ** 2 > 2 ** 32
    b = hip.debug_quality(src, rec)
    assert _bits(a) == _bits(b)                       # deterministic, bit for bit


def _cropped(seq, t, sw, sh):
    y, u, v = seq.frame(t)
    return (np.ascontiguousarray(y[:sh, :sw]), np.ascontiguousarray(u[:sh // 2, :sw // 2]), np.ascontiguousarray(v[:sh // 2, :sw // 2]))


@pytest.mark.parametrize("lf_type", [0, 1])
def test_every_frames_record_is_the_reconstruction_against_the_source(lf_type):
    """1280x720 coded, 1278x714 handed in: key and inter frames; stats on and off give the same bytes and reconstructions"""
    W, H, sw, sh = 1280, 720, 1278, 714
    seq = SynthSequence(W, H, seed=11)
    cfg = dict(gop_size=3, num_partitions=2, src_width=sw, src_height=sh, loop_filter_type=lf_type)
    on, off = api.NativeDriver(W, H, quality_stats=1, **cfg), api.NativeDriver(W, H, **cfg)
    with pytest.raises(api.Vp8HipError):
        off.frame_quality()
    records = []
    for t in range(5):
        src = _cropped(seq, t, sw, sh)
        d = [api.to_device(p) for p in src]
        api.device_synchronize()
        for drv in (on, off):
            drv.encode_frame_device(*(x.data_ptr() for x in d))
        a, b = on.get_frame(), off.get_frame()
        assert a == b, t
        rec_on, rec_off = on.hip.download_last(), off.hip.download_last()
        for p_, q_ in zip(rec_on, rec_off):
            assert np.array_equal(p_, q_), t
        q = on.frame_quality()
        assert q.frame_number == t and q.is_key == (t % 3 == 0), (t, q.frame_number, q.is_key)
        _same(q, frame_stats(src, rec_on, sw, sh), t)
        records.append(q)
    s = on.quality_summary()
    assert s.frames == 5
    assert list(s.sse) == [sum(r.sse[p] for r in records) for p in range(3)]
    assert s.psnr_avg == pytest.approx(np.mean([r.psnr_all for r in records]), rel=1e-12)
    assert s.ssim_all == pytest.approx(np.mean([r.ssim_all for r in records]), rel=1e-12)
    k = int(np.argmin([r.psnr_all for r in records]))
    assert s.psnr_min == records[k].psnr_all and s.psnr_min_frame == k
    on.close()
    off.close()


def test_a_frame_sent_back_as_a_key_frame_has_the_key_frames_record():
    """tests/test_gpu_check_async.py's sequence (320x192, qi 50..110, target 0.90, a scene cut): the redone frame's record is the key
    frame's, and the summary counts every frame once"""
    W, H = 320, 192
    a, b = SynthSequence(W, H, seed=41), SynthSequence(W, H, seed=97)
    frames = [a.frame(t) for t in range(4)] + [b.frame(t) for t in range(4)]
    drv = api.NativeDriver(W, H, num_partitions=2, check_ssim=1, device_params=1, gop_size=150, qi_min=50, qi_max=110, ssim_target=0.90,
                           quality_stats=1)
    records = []
    for t, f in enumerate(frames):
        d = [api.to_device(p) for p in f]
        api.device_synchronize()
        drv.encode_frame_device(*(x.data_ptr() for x in d))
        key = drv.resolve()
        q = drv.frame_quality()
        assert q.frame_number == t and q.is_key == int(key), t
        _same(q, frame_stats(f, drv.hip.download_last(), W, H), t)
        records.append(q)
    st = drv.stats()
    assert st.redone_as_key >= 1
    s = drv.quality_summary()
    assert s.frames == len(frames)
    assert list(s.sse) == [sum(r.sse[p] for r in records) for p in range(3)]
    assert s.psnr_avg == pytest.approx(np.mean([r.psnr_all for r in records]), rel=1e-12)
    drv.close()


def _records_alone(W, H, cfg, ptrs):
    drv = api.NativeDriver(W, H, quality_stats=1, **cfg)
    out = []
    for p in ptrs:
        drv.encode_frame_device(*p)
        drv.get_frame()
        out.append(drv.frame_quality())
    s = drv.quality_summary()
    drv.close()
    return out, s


def _summary_of(records, s, what):
    assert s.frames == len(records), what
    assert list(s.sse) == [sum(r.sse[p] for r in records) for p in range(3)], what
    assert s.psnr_avg == pytest.approx(np.mean([r.psnr_all for r in records]), rel=1e-12), what
    assert s.ssim_all == pytest.approx(np.mean([r.ssim_all for r in records]), rel=1e-12), what


def test_batch_members_batches_and_the_video_loop_give_the_records_of_the_frame_by_frame_run():
    W, H, nd, frames = 320, 192, 6, 6
    seq = SynthSequence(W, H, seed=71)
    dev = [tuple(api.to_device(p) for p in seq.frame(t)) for t in range(nd)]
    api.device_synchronize()
    ptr = [tuple(p.data_ptr() for p in f) for f in dev]
    cfg = dict(gop_size=4, altref_range=2, num_partitions=2, device_params=1, check_ssim=1, qi_min=40, qi_max=110, ssim_target=0.92)
    # a batch of six, stats on for every other member: each member's records are those of its chunk coded alone
    members = [api.NativeDriver(W, H, quality_stats=int(i % 2 == 0), **cfg) for i in range(6)]
    nb = api.NativeBatch(members)
    got = [[] for _ in members]
    for t in range(frames):
        nb.encode_frame_device([ptr[(i + t) % nd] for i in range(6)])
        for i, m in enumerate(members):
            m.get_frame()
            if i % 2 == 0:
                got[i].append(m.frame_quality())
            else:
                with pytest.raises(api.Vp8HipError):
                    m.frame_quality()
    for i in range(0, 6, 2):
        alone, s = _records_alone(W, H, cfg, [ptr[(i + t) % nd] for t in range(frames)])
        assert [_bits(q) for q in got[i]] == [_bits(q) for q in alone], i
        _summary_of(alone, members[i].quality_summary(), i)
    nb.close()
    for m in members:
        m.close()
    # two batches of three on a host thread each, frames out
    starts = [[0, 2, 4], [1, 3, 5]]
    rows = [[api.NativeDriver(W, H, quality_stats=1, **cfg) for _ in r] for r in starts]
    nbs = [api.NativeBatch(r) for r in rows]
    api.NativeBatch.encode_frames_device_all(nbs, frames, ptr, starts, frames_out=True)
    for k, r in enumerate(starts):
        for i, s0 in enumerate(r):
            alone, _ = _records_alone(W, H, cfg, [ptr[(s0 + t) % nd] for t in range(frames)])
            _summary_of(alone, rows[k][i].quality_summary(), (k, i))
    for nb in nbs:
        nb.close()
    for r in rows:
        for d in r:
            d.close()
    # the native video loop, with and without frames out
    alone, _ = _records_alone(W, H, cfg, [ptr[t % nd] for t in range(frames)])
    for with_out in (True, False):
        drv = api.NativeDriver(W, H, quality_stats=1, **cfg)
        if with_out:
            drv.encode_video_device(frames, ptr)
        else:
            drv.encode_video_device_no_frames(frames, ptr)
        _summary_of(alone, drv.quality_summary(), with_out)
        drv.close()


def test_overlap_filter_with_frames_staged_early_keeps_every_record():
    W, H = 320, 192
    seq = SynthSequence(W, H, seed=5)
    frames = [tuple(np.ascontiguousarray(p) for p in seq.frame(t)) for t in range(6)]
    cfg = dict(gop_size=4, num_partitions=2, check_ssim=1, qi_min=40, qi_max=110, ssim_target=0.92)
    drv = api.NativeDriver(W, H, quality_stats=1, overlap_filter=1, **cfg)
    drv.lib.vp8drv_stage_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    records = []
    for t, f in enumerate(frames):
        drv.encode_frame_host(*f)
        drv.get_frame()
        q = drv.frame_quality()
        assert q.frame_number == t
        _same(q, frame_stats(f, drv.hip.download_last(), W, H), t)
        records.append(q)
        if t + 1 < len(frames):
            assert drv.lib.vp8drv_stage_frame_host(drv.h, *(p.ctypes.data for p in frames[t + 1])) == 0
    _summary_of(records, drv.quality_summary(), "overlap")
    drv.close()
