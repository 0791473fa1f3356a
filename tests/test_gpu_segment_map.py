"""The per-macroblock quantiser on the device (vp8hip_set_segment_mode): the variance-adaptive map of k_aq_map_b + k_aq_seg_b against the
numpy rule of tests/aq_ref.py whichever way a frame comes in; the mapped macroblock kernels (k_mb_p_map, k_mb_p_map_conformant) against
the result assembled from the oracle's stages (tests/segment_map_ref.py); the native frame loop end to end (bytes, a decoder, the
analysis record, GOP chunks in a batch); every refusal; off is off.  Everything is exact: no tolerances (MB_SSIM by bit pattern)."""
import ctypes as C

import numpy as np
import pytest

import aq_ref
from pipeline import default_segments, load_meta

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4

# macroblocks of uniform noise around 128, four amplitudes in turn: with these the numpy rule alone gives every segment a macroblock at
# 80x48 and 176x144 (asserted below before the device is looked at); a ratio of 2 never reaches segment 0 at strength 1, a ratio of 4 does
AMPLITUDES = {1: (1, 4, 16, 64), 2: (3, 6, 12, 24), 3: (3, 6, 12, 24)}


def aq_frame(W, H, strength, seed):
    rng = np.random.default_rng(1000 + seed)
    y = aq_ref.noise_blocks(W, H, AMPLITUDES[strength], seed=seed)
    return y, rng.integers(96, 160, (H // 2, W // 2), dtype=np.uint8), rng.integers(96, 160, (H // 2, W // 2), dtype=np.uint8)


def expected_aq(y, strength):
    m, e, _ = aq_ref.aq_map(y, strength)
    if y.shape != (32, 48):      # 48x32 has six macroblocks: too few for the condition
        assert (np.bincount(m, minlength=4) > 0).all(), (y.shape, strength, np.bincount(m, minlength=4))
    return m, e


# ---- 1. the variance-adaptive map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["device", "upload", "prefetch"])
@pytest.mark.parametrize("size", [(48, 32), (80, 48), (176, 144)])      # one partial group of four; five wide; 99 macroblocks
def test_aq_map_equals_the_rule(size, way):
    from test_gpu_analysis import current_luma, take
    from vp8oclenc_amd import api
    W, H = size
    hip = api.Vp8Hip(W, H)
    keep = []
    for strength in (1, 2, 3, 2):
        hip.set_segment_mode(2, strength)
        assert hip.segment_mode() == (2, strength)
        f = aq_frame(W, H, strength, seed=W + strength + len(keep))
        want_m, want_e = expected_aq(f[0], strength)
        take(hip, f, way, keep)
        assert np.array_equal(current_luma(hip), f[0])
        m, e = hip.download_segment_map(with_e=True)
        assert np.array_equal(e, want_e), (size, way, strength)
        assert np.array_equal(m, want_m), (size, way, strength)
    hip.close()


def test_aq_map_of_a_padded_source_counts_the_padding():
    from test_gpu_analysis import current_luma
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(48, 32)
    hip.set_source_size(40, 24)
    hip.set_segment_mode(2, 3)
    y, u, v = aq_frame(48, 32, 3, seed=5)
    hip.upload_current(np.ascontiguousarray(y[:24, :40]), np.ascontiguousarray(u[:12, :20]), np.ascontiguousarray(v[:12, :20]))
    cur = current_luma(hip)
    assert cur.shape == (32, 48) and np.array_equal(cur[:24, :40], y[:24, :40])
    want_m, want_e, _ = aq_ref.aq_map(cur, 3)
    m, e = hip.download_segment_map(with_e=True)
    assert np.array_equal(e, want_e) and np.array_equal(m, want_m)
    hip.close()


def test_aq_map_in_a_batch_of_two_members_with_different_frames():
    from vp8oclenc_amd import api
    W, H = 80, 48
    drvs = [api.NativeDriver(W, H, gop_size=4, altref_range=2) for _ in range(2)]
    for d in drvs:
        d.set_segment_mode(2, 2)
    b = api.NativeBatch(drvs)
    for t in range(3):
        frames = [aq_frame(W, H, 2, seed=10 * t + i) for i in range(2)]
        want = [expected_aq(f[0], 2) for f in frames]
        assert not np.array_equal(want[0][1], want[1][1])
        dev = [[api.to_device(p) for p in f] for f in frames]
        keys = b.encode_frame_device([tuple(x.data_ptr() for x in d) for d in dev])
        for i, d in enumerate(drvs):
            m, e = d.hip.download_segment_map(with_e=True)
            assert np.array_equal(e, want[i][1]) and np.array_equal(m, want[i][0]), (t, i)
            seg = d.hip.download_results(recon=False)["MB_segment_id"]
            assert np.array_equal(seg, np.zeros_like(seg) if keys[i] else want[i][0]), (t, i)
        b.get_frames_begin()
        for d in drvs:
            d.get_frame_end()
    b.close()
    for d in drvs:
        d.close()


# ---- 2. the mapped macroblock kernels against the assembled oracle ------------------------------------------------------------------
KEYS = ["MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs", "MB_segment_id", "MB_SSIM", "prefilter_Y", "prefilter_U", "prefilter_V",
        "MB_non_zero_coeffs", "mb_mask", "recon_Y", "recon_U", "recon_V"]


def mb_case(name):
    """-> (frames [LAST, GOLDEN, ALTREF, current], flags, segment data)"""
    import os
    from vp8oclenc_amd.synth import SynthSequence
    if name == "96x64_3refs":
        z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g96x64_3refs.npz"))
        meta = load_meta(z)
        cur = tuple(np.ascontiguousarray(z[f"in_cur_{p}"]) for p in "YUV")
        refs = [tuple(np.ascontiguousarray(z[f"in_ref{r}_{p}"]) for p in "YUV") for r in range(3)]
        return refs + [cur], (meta["use_golden"], meta["use_altref"]), np.asarray(z["segments"])
    W, H, flags, seed = {"80x48_last_only": (80, 48, (0, 0), 4), "176x144": (176, 144, (1, 1), 7)}[name]
    s = SynthSequence(W, H, seed=seed, noise=6)
    f = [s.frame(t) for t in range(4)]
    return [f[2], f[0], f[1], f[3]], flags, default_segments()


def maps_for(mbs):
    rng = np.random.default_rng(mbs)
    four_in_a_group = np.full(mbs, 3, np.uint8)
    four_in_a_group[:4] = [2, 0, 3, 1]      # (a workgroup takes eight consecutive macroblocks: all four segments inside the first)
    if mbs > 8:
        four_in_a_group[-3:] = [1, 2, 0]    # ... and inside the last, partly empty one
    return [("four in a group", four_in_a_group)] + [(f"constant {s}", np.full(mbs, s, np.uint8)) for s in range(4)] + \
           [("random", rng.integers(0, 4, mbs).astype(np.uint8))]


def device_frame(hip, frames, sd, flags):
    from vp8oclenc_amd import api
    hip.set_segments(sd)
    hip.upload_last(*frames[0])
    hip.upload_current(*frames[3])
    hip.inter_transform(0, 0, *flags)
    res = hip.download_results(recon=True)
    res["mb_mask"] = hip.debug(api.DBG_MB_MASK)      # the transform's own mask and counts (the frame loop filters with them as they are)
    res["MB_non_zero_coeffs"] = hip.debug(api.DBG_MB_NZ)
    hip.loop_filter()
    res["recon_Y"], res["recon_U"], res["recon_V"] = hip.download_last()
    return res


@pytest.mark.parametrize("conformant", [False, True], ids=["reference_predictor", "conformant"])
@pytest.mark.parametrize("name", ["96x64_3refs", "80x48_last_only", "176x144"])
def test_mapped_macroblock_kernel_equals_the_assembled_oracle(name, conformant):
    from oracle_lib import Oracle
    from segment_map_ref import run_mapped_inter_frame
    from test_gpu_parity import _compare
    from test_gpu_search_saturating import _prepare
    from vp8oclenc_amd import api
    frames, flags, sd = mb_case(name)
    H, W = frames[3][0].shape
    mbs = (W // 16) * (H // 16)
    st = Oracle.stages()
    hip = api.Vp8Hip(W, H)
    if conformant:
        hip.conformant_stream(True)
    hip.set_segments(sd)
    if flags != (0, 0):
        _prepare(hip, frames)
    mode0 = device_frame(hip, frames, sd, flags)
    assert (mode0["MB_segment_id"] == 3).all()
    Oracle.lib().vp8o_set_conformant_stream(int(conformant))
    try:
        hip.set_segment_mode(1)
        no_map = device_frame(hip, frames, sd, flags)      # mode 1 without a map: segment 3 everywhere, the default's frame
        _compare(no_map, mode0, KEYS, f"{name}: mode 1 without a map against mode 0")
        used = np.zeros(4, np.int64)
        for tag, seg_map in maps_for(mbs):
            hip.upload_segment_map(seg_map)
            assert np.array_equal(hip.download_segment_map(), seg_map)
            h = device_frame(hip, frames, sd, flags)
            o = run_mapped_inter_frame(st, frames[3], frames[:3], sd, flags[0], flags[1], seg_map)
            # block 24 exists only for 16x16 macroblocks: in a split one the device keeps what an earlier frame of the context left
            # there (the frames that made GOLDEN and ALTREF), the assembly starts from zeros, and nothing reads either
            split = h["MB_parts"] != 0
            assert np.array_equal(split, o["MB_parts"] != 0)
            stale = h["MB_coeffs"][split, 24].copy()
            h["MB_coeffs"][split, 24] = 0
            assert not o["MB_coeffs"][split, 24].any()
            _compare(h, o, KEYS, f"{name} {tag}{' conformant' if conformant else ''}")
            used += np.bincount(h["MB_segment_id"], minlength=4)
            h["MB_coeffs"][split, 24] = stale
            if tag == "constant 3":
                _compare(h, mode0, KEYS, f"{name}: the constant map 3 against mode 0 of the same context")
            if tag == "constant 0":
                assert not np.array_equal(h["MB_coeffs"], mode0["MB_coeffs"])      # (the map is no no-op)
        assert (used > 0).all()
        hip.set_segment_mode(0)
        _compare(device_frame(hip, frames, sd, flags), mode0, KEYS, f"{name}: mode 0 again")
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)
    hip.close()


# ---- 3. the driver end to end -----------------------------------------------------------------------------------------------------
def driver_frames(W, H, n):
    """a panning picture under macroblock noise of four amplitudes: motion for the searches, every segment for mode 2"""
    from vp8oclenc_amd.synth import SynthSequence
    s = SynthSequence(W, H, seed=77)
    out = []
    for t in range(n):
        y, u, v = s.frame(t)
        noise = aq_ref.noise_blocks(W, H, (0, 5, 20, 80), seed=3).astype(np.int32) - 128      # (the same noise every frame: it is predicted)
        out.append((np.clip(y.astype(np.int32) // 2 + 64 + noise, 0, 255).astype(np.uint8), u, v))
    return out


def setup_mode(drv, mode, seg_map):
    if mode == 1:
        drv.set_segment_mode(1)
        drv.set_segment_map(seg_map)
    else:
        drv.set_segment_mode(2, 2)


@pytest.mark.parametrize("mode", [1, 2])
def test_driver_end_to_end(mode):
    from bitstream_cases import expected_frame
    from test_decode_roundtrip import _decode_sequence
    from test_gpu_analysis import current_luma
    from vp8oclenc_amd import api
    W, H, N = 80, 48, 6
    mbs = (W // 16) * (H // 16)
    frames = driver_frames(W, H, N)
    seg_map = np.random.default_rng(8).integers(0, 4, mbs).astype(np.uint8)
    cfg = dict(gop_size=4, altref_range=2, conformant_stream=1, num_partitions=1)
    drv = api.NativeDriver(W, H, **cfg)
    setup_mode(drv, mode, seg_map)
    drv.set_analysis(True)
    serial, keys, hist = [], [], np.zeros(4, np.int64)

    def run():
        for t, f in enumerate(frames):
            key = drv.encode_frame_host(*f)
            frame = drv.get_frame()
            key = bool(drv.resolve()) or bool(key)
            res = drv.hip.download_results(recon=False)
            want_map = seg_map if mode == 1 else aq_ref.aq_map(current_luma(drv.hip), 2)[0]
            if mode == 2:
                assert np.array_equal(drv.hip.download_segment_map(), want_map), t
            seg = np.zeros(mbs, np.int64) if key else want_map.astype(np.int64)
            assert np.array_equal(res["MB_segment_id"], seg), t
            r = drv.frame_analysis()
            assert list(r.segment_mbs) == np.bincount(seg, minlength=4).tolist() and r.is_key == int(key), t
            if not key:
                hist[:] += np.bincount(seg, minlength=4)
            # the host form of the frame (vp8bs_*, through bitstream_cases.expected_frame) fed with what the device holds
            sd, _, sharp = drv.hip.get_segments()
            st = drv.stats()
            if not key and st.last_min_ssim > np.float32(0.95):      # check_SSIM's filter update on the device (vp8enc.cpp:260-261)
                sharp = 7
            res.update(segments=sd, sharpness=sharp, is_altref=int(st.last_was_altref))
            if key:
                res["modes"] = drv.hip.download_intra()[0]
            assert frame == expected_frame(W, H, res, key, 1, use_reference=False), f"frame {t}: not the host form's bytes"
            serial.append(frame)
            keys.append(key)
            yield frame, key, drv.hip.download_last()

    seen = _decode_sequence(run(), f"mode {mode}")
    assert keys == [True, False, False, False, True, False] and seen["inter_frames"] == 4
    assert (hist > 0).all(), hist      # the inter frames used every segment
    drv.close()
    # the same six frames as two GOP chunks in one batch: the serial program's bytes
    chunks = [api.NativeDriver(W, H, **cfg) for _ in range(2)]
    for d in chunks:
        setup_mode(d, mode, seg_map)
    b = api.NativeBatch(chunks)
    dev = [[api.to_device(p) for p in f] for f in frames]
    ptr = [tuple(x.data_ptr() for x in d) for d in dev]
    got = [[], []]
    for t in range(4):
        on = [True, t < 2]
        b.encode_frame_device([ptr[t], ptr[4 + t] if t < 2 else None], on)
        b.get_frames_begin(on)
        for i, d in enumerate(chunks):
            if on[i]:
                got[i].append(d.get_frame_end())
    assert got[0] + got[1] == serial
    b.close()
    for d in chunks:
        d.close()


# ---- 4. the refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from vp8oclenc_amd import api
    W, H = 48, 32
    mbs = 6
    hip = api.Vp8Hip(W, H)
    lib = hip.lib
    lib.vp8hip_set_segment_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8hip_upload_segment_map.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_set_segment_map_device.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_download_segment_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    buf = np.zeros(mbs, np.uint8)
    assert lib.vp8hip_download_segment_map(hip.h, buf.ctypes.data, None) == ERR_STATE      # mode 0
    hip.set_segment_mode(2, 3)
    assert lib.vp8hip_download_segment_map(hip.h, buf.ctypes.data, None) == ERR_STATE      # mode 2, nothing taken in since
    for bad in ((3, 1), (-1, 0), (2, 0), (2, 4), (2, -1)):
        assert lib.vp8hip_set_segment_mode(hip.h, *bad) == ERR_ARG, bad
        assert hip.segment_mode() == (2, 3)
    assert lib.vp8hip_set_segment_mode(None, 1, 0) == ERR_ARG
    assert lib.vp8hip_upload_segment_map(hip.h, None) == ERR_ARG and lib.vp8hip_set_segment_map_device(hip.h, None) == ERR_ARG
    hip.set_segment_mode(1, 9)      # (modes 0 and 1 do not look at the strength)
    assert hip.segment_mode() == (1, 0)
    assert lib.vp8hip_download_segment_map(hip.h, buf.ctypes.data, buf.ctypes.data) == ERR_STATE      # e outside mode 2
    good = np.array([0, 1, 2, 3, 2, 1], np.uint8)
    hip.upload_segment_map(good)
    too_large = good.copy()
    too_large[4] = 4
    assert lib.vp8hip_upload_segment_map(hip.h, too_large.ctypes.data) == ERR_ARG
    assert np.array_equal(hip.download_segment_map(), good)      # the map in force is the one before
    d_map = api.to_device(np.array([3, 2, 1, 0, 1, 2], np.uint8))
    hip.set_segment_map_device(d_map.data_ptr())
    assert np.array_equal(hip.download_segment_map(), [3, 2, 1, 0, 1, 2])
    hip.close()
    # a context with an SSIM target: the ladder owns the segment id
    t = api.Vp8Hip(W, H, 0.9)
    assert lib.vp8hip_set_segment_mode(t.h, 1, 0) == ERR_STATE and lib.vp8hip_set_segment_mode(t.h, 2, 2) == ERR_STATE
    assert lib.vp8hip_upload_segment_map(t.h, good.ctypes.data) == ERR_STATE
    assert t.segment_mode() == (0, 0) and lib.vp8hip_set_segment_mode(t.h, 0, 0) == 0
    t.close()
    t0 = api.Vp8Hip(W, H, 0.0)
    assert lib.vp8hip_set_segment_mode(t0.h, 1, 0) == ERR_STATE
    t0.close()


def test_a_context_in_a_by_reference_split_is_refused_and_the_other_way_round():
    from vp8oclenc_amd import api, ref_shard
    W, H = 48, 32
    good = np.array([0, 1, 2, 3, 2, 1], np.uint8)
    lib = api.load_library()
    lib.vp8hip_set_segment_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8hip_upload_segment_map.argtypes = [C.c_void_p, C.c_void_p]
    be = ref_shard.HipRefBackend(W, H)
    be.shard_init(ref_shard.shard_unique_id(), 0, 1)
    assert lib.vp8hip_set_segment_mode(be.h, 1, 0) == ERR_STATE and lib.vp8hip_upload_segment_map(be.h, good.ctypes.data) == ERR_STATE
    assert be.segment_mode() == (0, 0)
    be.close()
    be = ref_shard.HipRefBackend(W, H)
    be.set_segment_mode(1)
    assert lib.vp8hip_shard_init(be.h, ref_shard.shard_unique_id(), 0, 1) == ERR_STATE and be.shard_world() == 0
    be.close()


def test_batch_members_must_agree_and_the_driver_refuses_what_the_library_refuses():
    from vp8oclenc_amd import api
    W, H = 48, 32
    drvs = [api.NativeDriver(W, H) for _ in range(2)]
    lib = drvs[0].lib
    lib.vp8drv_set_segment_mode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8drv_set_segment_map.argtypes = [C.c_void_p, C.c_void_p]
    for bad in ((3, 1), (-1, 0), (2, 0), (2, 4)):
        assert lib.vp8drv_set_segment_mode(drvs[0].h, *bad) == ERR_ARG
    assert lib.vp8drv_set_segment_map(drvs[0].h, None) == ERR_ARG
    assert lib.vp8drv_set_segment_map(drvs[0].h, np.full(6, 4, np.uint8).ctypes.data) == ERR_ARG
    assert drvs[0].hip.segment_mode() == (0, 0)
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    ctxs = (C.c_void_p * 2)(drvs[0].hip.h.value, drvs[1].hip.h.value)
    hb = C.c_void_p()
    for a, b_ in (((2, 2), (0, 0)), ((2, 2), (2, 3)), ((1, 0), (2, 1))):
        drvs[0].set_segment_mode(*a)
        drvs[1].set_segment_mode(*b_)
        with pytest.raises(api.Vp8HipError):
            api.NativeBatch(drvs)
        assert lib.vp8hip_batch_create(C.byref(hb), ctxs, 2) == ERR_ARG      # ... at the context level too
    drvs[0].set_segment_mode(1)
    drvs[1].set_segment_mode(1)
    b = api.NativeBatch(drvs)
    assert lib.vp8drv_set_segment_mode(drvs[0].h, 2, 2) == ERR_STATE      # a live batch member
    assert drvs[0].hip.segment_mode() == (1, 0)
    drvs[1].set_segment_map(np.array([0, 1, 2, 3, 0, 1], np.uint8))      # the maps are the members' own
    b.close()
    d = api.NativeDriver(W, H, ssim_target=0.9)
    assert lib.vp8drv_set_segment_mode(d.h, 1, 0) == ERR_STATE
    for x in drvs + [d]:
        x.close()


# ---- 5. off is off ----------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    from vp8oclenc_amd import api
    W, H = 80, 48
    frames = driver_frames(W, H, 3)
    cfg = dict(gop_size=150, altref_range=2, num_partitions=2)
    fresh, toggled, no_map = api.NativeDriver(W, H, **cfg), api.NativeDriver(W, H, **cfg), api.NativeDriver(W, H, **cfg)
    toggled.hip.set_segment_mode(2, 2)
    toggled.hip.set_segment_mode(0, 0)
    no_map.set_segment_mode(1)      # mode 1 without a map: segment 3 everywhere, exactly the default's frames
    for t, f in enumerate(frames):
        out = []
        for d in (fresh, toggled, no_map):
            d.encode_frame_host(*f)
            out.append(d.get_frame())
        assert out[0] == out[1], t
        assert out[0] == out[2], t
    for d in (fresh, toggled, no_map):
        d.close()


# ---- 6. the tools -----------------------------------------------------------------------------------------------------------------
def test_the_tools_take_the_mode(tmp_path):
    """-aq on scripts/native/y4m_to_ivf (one video, the filter on its own stream), on y4m_to_ivf_gops (GOP chunks in a batch) and --aq on
    scripts/encode_ivf.py write the same file, which is not the default's; --segment-map is the driver's mode 1"""
    import os
    import shutil
    import subprocess
    import sys
    from vp8oclenc_amd import api, y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exes = {}
    for name in ("y4m_to_ivf", "y4m_to_ivf_gops"):
        exes[name] = str(tmp_path / name)
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "scripts", "native", name + ".cpp"), "-o", exes[name],
                        "-L", os.path.join(root, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(root, "vp8oclenc_amd")], check=True, timeout=300)
    W, H, N = 80, 48, 6
    frames = driver_frames(W, H, N)
    src = str(tmp_path / "in.y4m")
    y4m.write_y4m(src, frames, framerate=25)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr

    def out(name):
        return open(tmp_path / name, "rb").read()
    run([exes["y4m_to_ivf"], src, str(tmp_path / "plain.ivf"), "-g", "3", "-no-scene-detect"])
    run([exes["y4m_to_ivf"], src, str(tmp_path / "aq.ivf"), "-g", "3", "-no-scene-detect", "-aq", "2"])
    run([exes["y4m_to_ivf_gops"], src, str(tmp_path / "aq_gops.ivf"), "-g", "3", "-aq", "2", "-chunks", "2", "-batch", "2"])
    encode_ivf = [sys.executable, os.path.join(root, "scripts", "encode_ivf.py")]
    run(encode_ivf + [str(tmp_path / "aq_py.ivf"), "--y4m", src, "--frames", str(N), "--gop", "3", "--aq", "2"])
    assert out("aq.ivf") != out("plain.ivf")
    assert out("aq.ivf") == out("aq_gops.ivf")
    assert out("aq.ivf") == out("aq_py.ivf")
    # the file equals the driver's frames in mode 2
    drv = api.NativeDriver(W, H, gop_size=3)
    drv.set_segment_mode(2, 2)
    got = []
    for f in frames:
        drv.encode_frame_host(*f)
        got.append(drv.get_frame())
    drv.close()
    data = out("aq.ivf")
    pos, packets = 32, []
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "little")
        packets.append(data[pos + 12:pos + 12 + n])
        pos += 12 + n
    assert packets == got
    # --segment-map: the same map for every frame
    seg_map = np.random.default_rng(4).integers(0, 4, (W // 16) * (H // 16)).astype(np.uint8)
    seg_map.tofile(str(tmp_path / "map.bin"))
    run(encode_ivf + [str(tmp_path / "map.ivf"), "--y4m", src, "--frames", str(N), "--gop", "3", "--segment-map", str(tmp_path / "map.bin")])
    drv = api.NativeDriver(W, H, gop_size=3)
    drv.set_segment_mode(1)
    drv.set_segment_map(seg_map)
    got = []
    for f in frames:
        drv.encode_frame_host(*f)
        got.append(drv.get_frame())
    drv.close()
    data = out("map.ivf")
    pos, packets = 32, []
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "little")
        packets.append(data[pos + 12:pos + 12 + n])
        pos += 12 + n
    assert packets == got
    (tmp_path / "bad.bin").write_bytes(bytes([4] * seg_map.size))
    r = subprocess.run(encode_ivf + [str(tmp_path / "bad.ivf"), "--y4m", src, "--frames", "2", "--segment-map", str(tmp_path / "bad.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0
