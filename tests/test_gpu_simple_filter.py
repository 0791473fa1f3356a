"""The simple loop filter on the device (vp8hip_set_loop_filter_type 1, vp8drv_config.loop_filter_type = 1, kernels_lf_simple.hip)
against the RFC 6386 section 15.2 restatement (tests/vp8_decode_simple.py) and libwebp."""
import numpy as np
import pytest

import webp_decode
from pipeline import default_segments
from test_simple_filter_cpu import restate, skip_inner_of
from vp8_decode_simple import SimpleFilterDecoder
from vp8oclenc_amd import api
from vp8oclenc_amd.synth import SynthSequence

pytestmark = pytest.mark.gpu
needs_libwebp = pytest.mark.skipif(webp_decode.libwebp() is None, reason="no libwebp in this image")


def _same(planes, recon, what):
    for name, a, b in zip("YUV", planes, recon):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        n = int((a != b).sum())
        assert n == 0, f"{what}: plane {name} differs in {n} samples"


def _inputs(W, H, seed):
    """lf_check.py's setup: smooth-ish content the filter acts on, random coefficients, partitions and segments"""
    rng = np.random.default_rng(seed)
    mbs = (W // 16) * (H // 16)
    base = rng.integers(0, 256, size=(H // 8 + 2, W // 8 + 2)).astype(np.float32)
    y = np.kron(base, np.ones((8, 8), np.float32))[:H, :W] + rng.integers(-6, 7, size=(H, W))
    y = np.clip(y * 1.3 - 30, 0, 255).astype(np.uint8)
    u = rng.integers(0, 256, size=(H // 2, W // 2)).astype(np.uint8)
    v = np.ascontiguousarray(u[::-1, ::-1])
    coeffs = np.zeros((mbs, 25, 16), np.int16)
    coeffs[rng.random(mbs) < 0.6, 3, 5] = 7
    coeffs[rng.random(mbs) < 0.2, 24, 0] = 3       # a Y2 DC only: counts for a whole macroblock, not for a split one
    parts = (rng.random(mbs) < 0.3).astype(np.int32)
    seg = rng.integers(0, 4, size=mbs).astype(np.int32)
    return y, u, v, coeffs, parts, seg


def _filter_alone(W, H, seed, levels=(6, 10, 14, 20), launches=3):
    y, u, v, coeffs, parts, seg = _inputs(W, H, seed)
    sd = default_segments(lf_levels=levels)
    want = restate(y, sd, seg, skip_inner_of(coeffs, parts), W // 16, H // 16)
    hip = api.Vp8Hip(W, H)
    hip.set_segments(sd)
    hip.upload_mb_data(coeffs, parts, seg)
    hip.set_loop_filter_type(1)
    got = []
    for _ in range(launches):   # hand-off races show up as launch-to-launch differences
        hip.upload_recon(y, u, v)
        hip.prepare_filter_mask(want_nz=False)
        hip.loop_filter()
        got.append(hip.download_last())
    hip.close()
    for k, (gy, gu, gv) in enumerate(got):
        d = np.argwhere(gy != want)
        assert len(d) == 0, f"{W}x{H} launch {k}: Y differs in {len(d)} samples, first (y, x) {d[:4].tolist()}"
        assert np.array_equal(gu, u) and np.array_equal(gv, v), f"{W}x{H} launch {k}: chroma was touched"
    return y, want, seg


@pytest.mark.parametrize("W,H", [(16, 16), (16, 48), (32, 64), (16, 272), (240, 112), (320, 240), (48, 16), (272, 16),
                                 (128, 128), (2048, 128), (16, 2160), (1920, 1088), (3840, 2160)])
def test_simple_filter_alone_on_band_and_ring_edge_geometries(W, H):
    y, want, _ = _filter_alone(W, H, seed=W + H)
    if W * H >= 128 * 128:
        assert (want != y).any()


def test_level_zero_skips_the_macroblock_and_filters_the_rest():
    W, H = 256, 144
    y, want, seg = _filter_alone(W, H, seed=8, levels=(6, 0, 14, 20))
    mbw = W // 16
    first0 = int(np.argmax(seg == 1))
    after = [mb for mb in range(first0 + 1, len(seg)) if seg[mb] != 1]
    changed = lambda mb: (want[(mb // mbw) * 16:(mb // mbw) * 16 + 16, (mb % mbw) * 16:(mb % mbw) * 16 + 16] !=
                          y[(mb // mbw) * 16:(mb // mbw) * 16 + 16, (mb % mbw) * 16:(mb % mbw) * 16 + 16]).any()
    assert any(changed(mb) for mb in after), "macroblocks after a level-0 one must still be filtered"


def test_set_loop_filter_type_rejects_other_values():
    hip = api.Vp8Hip(64, 48)
    for t in (-1, 2, 3):
        with pytest.raises(api.Vp8HipError):
            hip.set_loop_filter_type(t)
    hip.set_loop_filter_type(1)
    hip.set_loop_filter_type(0)
    hip.close()
    with pytest.raises(api.Vp8HipError):
        api.NativeDriver(64, 48, loop_filter_type=2)


@needs_libwebp
@pytest.mark.parametrize("W,H,seed", [(176, 144, 1), (640, 352, 3), (1920, 1080, 5), (3840, 2160, 6)])
def test_key_frames_decode_by_libwebp(W, H, seed):
    import vp8_parse
    s = SynthSequence(W, H, seed=seed)
    drv = api.NativeDriver(s.W, s.H, gop_size=3, num_partitions=4, loop_filter_type=1)
    keys = 0
    for t in range(4):
        drv.encode_frame_host(*s.frame(t))
        frame = drv.get_frame()
        if drv.resolve():
            keys += 1
            assert vp8_parse.parse_frame(frame, vp8_parse.StreamState()).filter_type == 1
            _same(webp_decode.decode_key_frame(frame), drv.hip.download_last(), f"{W}x{H} frame {t}")
    assert keys == 2
    drv.close()


@pytest.mark.parametrize("W,H,seed,frames,P,cfg", [
    (176, 144, 1, 8, 1, dict(gop_size=5, altref_range=2, device_params=0)),
    (320, 192, 4, 7, 4, dict(gop_size=6, altref_range=2, check_ssim=1, ssim_target=0.92, qi_min=40, qi_max=110, device_params=1)),
    (640, 352, 3, 6, 8, dict(gop_size=150, altref_range=3, check_ssim=1, device_params=1)),
    (336, 256, 2, 6, 4, dict(gop_size=4, altref_range=2, check_ssim=1, ssim_target=0.97, qi_min=0, qi_max=20, device_params=0)),
])
def test_sequences_decode_to_the_device_reconstruction(W, H, seed, frames, P, cfg):
    """conformant streams with golden / altref and check_SSIM (fallback and filter update): every frame, decoded from its bytes by
    the restatement, is the device's LAST"""
    s = SynthSequence(W, H, seed=seed)
    drv = api.NativeDriver(s.W, s.H, num_partitions=P, conformant_stream=1, loop_filter_type=1, **cfg)
    dec = SimpleFilterDecoder()
    for t in range(frames):
        drv.encode_frame_host(*s.frame(t))
        frame = drv.get_frame()
        drv.resolve()
        f, planes = dec.decode(frame)
        assert f.filter_type == 1
        _same(planes, drv.hip.download_last(), f"{W}x{H} frame {t}")
    drv.close()


def _run(drv, s, frames):
    out = []
    for t in range(frames):
        drv.encode_frame_host(*s.frame(t))
        out.append(drv.get_frame())
    drv.resolve()
    return out


def test_overlap_filter_gives_the_same_bytes():
    s = SynthSequence(320, 192, seed=9)
    cfg = dict(gop_size=5, altref_range=2, loop_filter_type=1, conformant_stream=1)
    a, b = api.NativeDriver(s.W, s.H, **cfg), api.NativeDriver(s.W, s.H, overlap_filter=1, **cfg)
    assert _run(a, s, 6) == _run(b, s, 6)
    a.close(); b.close()


def test_default_is_the_normal_filter_byte_for_byte():
    s = SynthSequence(320, 192, seed=10)
    a, b = api.NativeDriver(s.W, s.H, gop_size=4), api.NativeDriver(s.W, s.H, gop_size=4, loop_filter_type=0)
    assert _run(a, s, 5) == _run(b, s, 5)
    a.close(); b.close()


def test_switching_types_keeps_the_normal_filter_exact():
    """one context 0 -> 1 -> 0 between GOPs (the simple filter's band counters are its own): its type-0 frames are the bytes of
    a context that never switched"""
    s = SynthSequence(320, 192, seed=11)
    pure, sw = api.NativeDriver(s.W, s.H, gop_size=3), api.NativeDriver(s.W, s.H, gop_size=3)
    for t in range(9):
        if t in (3, 6):
            sw.hip.set_loop_filter_type(1 if t == 3 else 0)
        for d in (pure, sw):
            d.encode_frame_host(*s.frame(t))
        a, b = pure.get_frame(), sw.get_frame()
        if t < 3 or t >= 6:
            assert a == b, f"frame {t}"
    pure.close(); sw.close()


def test_batch_equals_single_contexts_and_refuses_mixed_types():
    seqs = [SynthSequence(320, 192, seed=k) for k in (1, 2, 3)]
    cfg = dict(gop_size=5, altref_range=2, num_partitions=2, device_params=1, check_ssim=1, conformant_stream=1, loop_filter_type=1)
    singles = [api.NativeDriver(320, 192, **cfg) for _ in seqs]
    members = [api.NativeDriver(320, 192, **cfg) for _ in seqs]
    batch = api.NativeBatch(members)
    for t in range(6):
        dev = [tuple(api.to_device(p) for p in s.frame(t)) for s in seqs]
        ptr = [tuple(p.data_ptr() for p in f) for f in dev]
        batch.encode_frame_device(ptr)
        batch.get_frames_begin()
        for i, d in enumerate(singles):
            d.encode_frame_device(*ptr[i])
            assert d.get_frame() == members[i].get_frame_end(), (t, i)
        api.device_synchronize()
    batch.close()
    normal = api.NativeDriver(320, 192, **dict(cfg, loop_filter_type=0))
    with pytest.raises(api.Vp8HipError):
        api.NativeBatch([members[0], normal])
    for d in singles + members + [normal]:
        d.close()
