"""Cyclic intra refresh on the device.  Context level: vp8hip_intra_refresh (k_intra_refresh) against the result assembled from the
oracle's existing stages (tests/refresh_ref.refresh_frame) -- coefficients, reconstruction, modes, is_inter, MB_parts, MB_segment_id,
non-zero counts and masks byte for byte, MB_SSIM bit pattern for bit pattern, and the loop-filtered frame behind it.  Driver level:
vp8drv_set_intra_refresh against the CPU oracle's frame loop with the rule (tests/refresh_ref.oracle_loop) -- every frame's bytes and
reconstruction, plain and with temporal layers, with a forced key frame, with the period set inside a GOP, both first-partition coders,
both intakes -- and, on a conformant stream, against the RFC 6386 decoder of tests/vp8_decode.py.  Off is off; every refusal.
Everything is exact: no tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest

import arf_ref
import refresh_ref as ref
import temporal_ref
from pipeline import default_segments

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
QI = dict(qi_min=10, qi_max=60)
KEYS = ["MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs", "MB_segment_id", "MB_SSIM", "prefilter_Y", "prefilter_U", "prefilter_V",
        "modes", "is_inter", "MB_non_zero_coeffs", "mb_mask", "recon_Y", "recon_U", "recon_V"]


# ---- 1. the context against the assembled oracle ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_frames(W, H):
    from vp8oclenc_amd.synth import SynthSequence
    s = SynthSequence(W, H, seed=W + H, noise=6)
    return s.frame(0), s.frame(1)


def mixed_map(mbs):
    m = np.random.default_rng(mbs).integers(0, 4, mbs).astype(np.uint8)
    m[:4] = [2, 0, 3, 1]
    return m


@functools.lru_cache(maxsize=None)
def oracle_inter(W, H, conformant, mode):
    """the oracle's inter frame of two_frames(W, H) (LAST only) -> its outputs; mode: 0 plain (tests/oracle_lib.Oracle), "map" /
    "aq": under a segment map, assembled from the oracle's stages (tests/segment_map_ref.py)"""
    from oracle_lib import Oracle
    last, cur = two_frames(W, H)
    sd = default_segments()
    Oracle.lib().vp8o_set_conformant_stream(int(conformant))
    try:
        if mode == 0:
            o = Oracle(W, H)
            o.set_segments(sd)
            o.upload_last(*last)
            o.upload_current(*cur)
            o.inter_transform(0, 0, 0, 0)
            res = o.download_results(recon=True)
            o.close()
            return res
        import aq_ref
        from segment_map_ref import run_mapped_inter_frame
        seg_map = mixed_map((W // 16) * (H // 16)) if mode == "map" else aq_ref.aq_map(cur[0], 2)[0]
        return run_mapped_inter_frame(Oracle.stages(), cur, [last, last, last], sd, 0, 0, seg_map)
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)


def expected_refresh(W, H, conformant, mode, P, q):
    from oracle_lib import Oracle
    last, cur = two_frames(W, H)
    sd = default_segments()
    o = oracle_inter(W, H, conformant, mode)
    Oracle.lib().vp8o_set_conformant_stream(int(conformant))
    try:
        e = ref.refresh_frame(cur, sd, o, P, q)
        e["MB_reference_frame"], e["MB_vectors"] = o["MB_reference_frame"], o["MB_vectors"]
        st = Oracle.stages()
        filt = [e["prefilter_" + p].copy() for p in "YUV"]
        sdf = np.ascontiguousarray(np.asarray(sd, np.int32).reshape(-1))
        seg = np.ascontiguousarray(e["MB_segment_id"], np.int32)
        for plane, (w, h, n) in zip(filt, ((W, H, 16), (W // 2, H // 2, 8), (W // 2, H // 2, 8))):
            st.loop_filter_frame(plane, seg, e["mb_mask"], sdf, w, h, n)
        e["recon_Y"], e["recon_U"], e["recon_V"] = filt
        return e
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)


def device_refresh(hip, W, H, P, q):
    from vp8oclenc_amd import api
    last, cur = two_frames(W, H)
    hip.set_segments(default_segments())
    hip.upload_last(*last)
    hip.upload_current(*cur)
    hip.inter_transform(0, 0, 0, 0)
    hip.intra_refresh(P, q)
    res = hip.download_results(recon=True)
    res["modes"], res["is_inter"] = hip.download_intra()
    res["mb_mask"] = hip.debug(api.DBG_MB_MASK)
    res["MB_non_zero_coeffs"] = hip.debug(api.DBG_MB_NZ)
    hip.loop_filter()      # no vp8hip_prepare_filter_mask in between: the refresh has renewed what it replaced
    res["recon_Y"], res["recon_U"], res["recon_V"] = hip.download_last()
    return res


def compare(h, e, what):
    from test_gpu_parity import _compare
    h, e = dict(h), dict(e)
    h["modes"], e["modes"] = np.asarray(h["modes"]).reshape(-1, 16), np.asarray(e["modes"]).reshape(-1, 16)
    # block 24 exists only for 16x16 macroblocks: elsewhere the device keeps what an earlier frame of the context left there and nothing reads it
    no_y2 = np.asarray(e["MB_parts"]) != 0
    assert np.array_equal(no_y2, np.asarray(h["MB_parts"]) != 0), what
    h["MB_coeffs"], e["MB_coeffs"] = h["MB_coeffs"].copy(), e["MB_coeffs"].copy()
    h["MB_coeffs"][no_y2, 24] = 0
    e["MB_coeffs"][no_y2, 24] = 0
    _compare(h, e, KEYS, what)


# 48x32 and 64x48 at P = 4: every phase hits row 0, column 0 and the last column (the 127 / 129 borders, the replicated above-right);
# 208x32 at P = 5: several forced macroblocks per row (the + P x stepping and the early exit: 13 columns, ceil(13 / 5) = 3 workgroups);
# 176x144 at P = 4, 7, 30: eleven columns, and at P = 30 phases at which some rows hold none; q >= P: the phase is taken modulo P
CASES = [(48, 32, 4, (0, 1, 2, 3, 6)), (64, 48, 4, (0, 1, 2, 3)), (208, 32, 5, (0, 1, 2, 3, 4)), (176, 144, 4, (1, 7)), (176, 144, 7, (0, 5)),
         (176, 144, 30, (0, 12, 26, 47))]


@pytest.mark.parametrize("W,H,P,phases", CASES, ids=[f"{c[0]}x{c[1]}-P{c[2]}" for c in CASES])
def test_refresh_equals_the_assembled_oracle(W, H, P, phases):
    """fails on a tree without the feature: there is no vp8hip_intra_refresh"""
    from vp8oclenc_amd import api
    mbw, mbh = W // 16, H // 16
    hip = api.Vp8Hip(W, H)
    empty_rows = 0
    for q in phases:
        e = expected_refresh(W, H, False, 0, P, q)
        fm = ref.forced_map(mbw, mbh, P, q)
        assert e["forced"] == api.intra_refresh_count(mbw, mbh, P, q) > 0
        empty_rows += int((~fm.any(axis=1)).sum())
        h = device_refresh(hip, W, H, P, q)
        assert np.array_equal(h["is_inter"] == 0, fm.reshape(-1)), (W, H, P, q)
        compare(h, e, f"{W}x{H} P={P} q={q}")
    if (W, P) == (176, 30):
        assert empty_rows > 0
    hip.close()


@pytest.mark.parametrize("mode", ["map", "aq", "conformant"])
def test_refresh_in_the_segment_the_inter_pass_left(mode):
    """a caller's map that mixes all four segments; the variance-adaptive map at strength 2; the conformant stream"""
    import aq_ref
    from vp8oclenc_amd import api
    W, H, P = 80, 48, 4
    mbs = (W // 16) * (H // 16)
    conformant = mode == "conformant"
    hip = api.Vp8Hip(W, H)
    if conformant:
        hip.conformant_stream(True)
    if mode == "map":
        hip.set_segment_mode(1)
        hip.upload_segment_map(mixed_map(mbs))
    elif mode == "aq":
        hip.set_segment_mode(2, 2)
    seen = set()
    for q in range(P):
        e = expected_refresh(W, H, conformant, 0 if conformant else mode, P, q)
        h = device_refresh(hip, W, H, P, q)
        if mode == "aq":
            assert np.array_equal(hip.download_segment_map(), aq_ref.aq_map(two_frames(W, H)[1][0], 2)[0])
        compare(h, e, f"{mode} q={q}")
        seen |= set(int(s) for s in h["MB_segment_id"][h["is_inter"] == 0])
    if mode == "map":
        assert seen == {0, 1, 2, 3}      # forced macroblocks of every segment
    hip.close()


def test_the_one_wavefront_form_computes_the_same():
    """VP8HIP_INTRA_REFRESH_1WAVE=1 (k_intra_refresh_1w: chroma and the source loads on the luma wavefront, no barriers) is read once
    per process, so a fresh interpreter runs context-level cases with it set: the borders, several forced macroblocks per row, empty
    rows, and every segment of a caller's map.  This test is about that second process."""
    import os
    import subprocess
    import sys
    if os.environ.get("VP8HIP_INTRA_REFRESH_1WAVE"):
        pytest.skip("this process runs the one-wavefront form already")
    here = os.path.abspath(__file__)
    env = dict(os.environ, VP8HIP_INTRA_REFRESH_1WAVE="1")
    cases = ["test_refresh_equals_the_assembled_oracle[48x32-P4]", "test_refresh_equals_the_assembled_oracle[208x32-P5]",
             "test_refresh_equals_the_assembled_oracle[176x144-P30]", "test_refresh_in_the_segment_the_inter_pass_left[map]"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + [f"{here}::{c}" for c in cases], env=env, capture_output=True,
                       text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(here)))
    assert r.returncode == 0 and "4 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_the_analysis_record_counts_the_forced_macroblocks_and_the_verdict_reports_none_replaced():
    from vp8oclenc_amd import api
    W, H, P, q = 64, 48, 4, 1
    last, cur = two_frames(W, H)
    refqi, _ = api.quantizer_ladders(10, 60)
    hip = api.Vp8Hip(W, H)
    hip.set_analysis(True)
    for refresh in (True, False, True):
        hip.set_segments(default_segments())
        hip.upload_last(*last)
        hip.upload_current(*cur)
        hip.inter_transform(0, 0, 0, 0)
        if refresh:
            hip.intra_refresh(P, q)
        hip.check_ssim_async(refqi, 10)
        hip.loop_filter()
        assert hip.check_ssim_result()[0] == 0      # a refresh is no replacement: nothing sends the frame back as a key frame
        a = hip.analysis_result()
        want = api.intra_refresh_count(W // 16, H // 16, P, q) if refresh else 0
        assert a.coded and a.mbs_intra == want and a.mbs_intra + sum(a.mbs_ref) == a.mbs_total, (refresh, a.mbs_intra)
    hip.close()


def test_every_refusal_of_the_context():
    from vp8oclenc_amd import api, ref_shard
    W, H = 64, 48
    last, cur = two_frames(W, H)
    lib = api.load_library()
    lib.vp8hip_intra_refresh.argtypes = [C.c_void_p, C.c_int, C.c_int]

    def inter(hip):
        hip.set_segments(default_segments())
        hip.upload_last(*last)
        hip.upload_current(*cur)
        hip.inter_transform(0, 0, 0, 0)

    hip = api.Vp8Hip(W, H)
    assert lib.vp8hip_intra_refresh(None, 4, 0) == ERR_ARG
    assert lib.vp8hip_intra_refresh(hip.h, 4, 0) == ERR_STATE      # no reconstruction in flight
    inter(hip)
    before = hip.download_results(recon=True)
    for period, q in ((0, 0), (1, 0), (3, 0), (1025, 0), (-4, 0), (4, -1)):
        assert lib.vp8hip_intra_refresh(hip.h, period, q) == ERR_ARG, (period, q)
    after = hip.download_results(recon=True)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    hip.intra_refresh(4, 0)      # ... and the frame is still there to be refreshed
    # the synchronous check_SSIM would initialise is_inter and modes over the forced macroblocks: refused, and they stand
    lib.vp8hip_check_ssim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    forced = hip.download_intra()[1].copy()
    assert (forced == 0).sum() == api.intra_refresh_count(W // 16, H // 16, 4, 0)
    assert lib.vp8hip_check_ssim(hip.h, None, None, None) == ERR_STATE
    assert np.array_equal(hip.download_intra()[1], forced)
    hip.loop_filter()
    assert lib.vp8hip_intra_refresh(hip.h, 4, 0) == ERR_STATE      # ended
    hip.close()
    # an SSIM target above -1: the ladder owns the segment id and its fallback the intra arrays
    for target in (-0.5, 0.0, 0.9):
        hip = api.Vp8Hip(W, H, target)
        inter(hip)
        before = hip.download_results(recon=True)
        assert lib.vp8hip_intra_refresh(hip.h, 4, 0) == ERR_STATE, target
        after = hip.download_results(recon=True)
        assert all(np.array_equal(before[k], after[k]) for k in before)
        hip.close()
    # a by-reference split (one rank is enough to make it one)
    be = ref_shard.HipRefBackend(W, H)
    inter(be)
    be.shard_init(ref_shard.shard_unique_id(), 0, 1)
    assert lib.vp8hip_intra_refresh(be.h, 4, 0) == ERR_STATE
    be.close()


# ---- 2. the driver against the oracle's loop ------------------------------------------------------------------------------------------------
TOTAL = 8
SCHEDULES = {"on": lambda t: 4, "off": lambda t: 0, "from frame 3": lambda t: 4 if t >= 3 else 0}


def same(got, want, what):
    for name, g, w in zip("YUV", got, want):
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


@functools.lru_cache(maxsize=None)
def pan(w, h):
    return arf_ref.noisy_pan(w, h, TOTAL, seed=w + TOTAL)


@functools.lru_cache(maxsize=None)
def oracle_records(w, h, layers, schedule, conformant, force_key=()):
    return ref.oracle_loop(pan(w, h), layers, SCHEDULES[schedule], conformant=bool(conformant), force_key=frozenset(force_key), gop_size=TOTAL,
                           altref_range=TOTAL + 1, check_ssim=True, **QI)


@functools.lru_cache(maxsize=None)
def expected_bytes(key, i, P):
    return temporal_ref.record_bytes(oracle_records(*key)[i], key[0], key[1], P)


def run_driver(key, P=1, way="host", first=0, compare=True, **cfg):
    """the native driver over the records' frames -> dict(stream, recons, infos, intra); asserts bytes, reconstructions, the refresh record
    and, on a conformant stream, the decoder's picture and the parsed intra set frame by frame"""
    from vp8oclenc_amd import api
    w, h, layers, schedule, conformant, force_key = key
    frames, recs = pan(w, h), oracle_records(*key)
    mbw, mbh = w // 16, h // 16
    drv = api.NativeDriver(w, h, gop_size=TOTAL, altref_range=TOTAL + 1, num_partitions=P, check_ssim=1, conformant_stream=conformant, **QI, **cfg)
    if layers > 1:
        drv.set_temporal_layers(layers, api.TL_KEEP_RECON)
    dec = None
    if conformant:
        import vp8_decode
        dec = vp8_decode.Decoder()
    dev = [[api.to_device(p) for p in f] for f in frames] if way == "device" else None
    if dev:
        api.device_synchronize()
    seen = dict(stream=[], recons=[], infos=[], intra=[])
    total = 0
    for t in range(first, len(frames)):
        r, what = recs[t], f"frame {t}"
        period = SCHEDULES[schedule](t)
        if t == first or period != SCHEDULES[schedule](t - 1):
            drv.set_intra_refresh(period)
        fk = t in force_key or t == first and first > 0
        if dev:
            was_key = drv.encode_frame_device(*(b.data_ptr() for b in dev[t]), force_key=fk)
        else:
            was_key = drv.encode_frame_host(*frames[t], force_key=fk)
        got = drv.get_frame()
        was_key = drv.resolve() or was_key
        info, layer = drv.intra_refresh(), drv.frame_layer()
        assert bool(was_key) == r["key"], what
        total += info.last_forced
        assert (info.period, info.last_forced, info.total_forced) == (period, r["refresh"]["forced"], total), (what, info.last_forced, r["refresh"])
        if first == 0:
            assert info.last_q == r["refresh"]["q"], (what, info.last_q, r["refresh"])
        if compare:
            exp = expected_bytes(key, t, P)
            assert len(got) == len(exp), f"{what}: {len(got)} bytes, expected {len(exp)}"
            if got != exp:
                a, b = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
                raise AssertionError(f"{what} differs at bytes {np.nonzero(a != b)[0][:8]} of {len(a)}")
        recon = drv.hip.download_last() if layer.refresh in (temporal_ref.LAST, temporal_ref.ALL) else drv.hip.refresh_frame()
        if compare:
            same(recon, r["recon"], what)
        refreshed = period and not r["key"] and layer.refresh == temporal_ref.LAST
        want = ref.forced_map(mbw, mbh, period, info.last_q).reshape(-1) if refreshed else np.zeros(mbw * mbh, bool)
        assert info.last_forced == int(want.sum()), what
        if dec is not None:
            f, planes = dec.decode(got)
            same(planes, recon, what + ": the decoder against the device")
            if not r["key"]:
                assert np.array_equal(f.is_inter == 0, want), what + ": the parsed intra set against the rule"
        seen["stream"].append(got)
        seen["recons"].append(recon)
        seen["infos"].append((info.last_q, info.last_forced, layer.refresh, bool(was_key)))
        seen["intra"].append(want)
    drv.close()
    for f in dev or ():
        for b in f:
            b.free()
    return seen


@pytest.mark.parametrize("host_bitstream,way,P", [(0, "host", 1), (1, "host", 2), (0, "device", 4)], ids=["device coder", "host coder", "device intake"])
@pytest.mark.parametrize("w,h", [(64, 48), (176, 144)])
def test_a_refreshing_driver_equals_the_oracle_loop(w, h, host_bitstream, way, P):
    """eight frames at P = 4, bytes and reconstructions; both first-partition coders, both intakes; fails on a tree without the feature"""
    seen = run_driver((w, h, 1, "on", 0, ()), P, way, host_bitstream=host_bitstream)
    assert [i[0] for i in seen["infos"]] == [0] + list(range(TOTAL - 1)) and all(i[1] > 0 for i in seen["infos"][1:])


@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("w,h", [(64, 48), (176, 144)])
def test_with_temporal_layers_only_frames_that_refresh_last_are_refreshed_and_counted(w, h, layers):
    seen = run_driver((w, h, layers, "on", 0, ()), 2)
    q = 0
    for t, (last_q, forced, refresh, key) in enumerate(seen["infos"]):
        if key:
            assert (last_q, forced) == (0, 0)
            continue
        assert last_q == q and (forced > 0) == (refresh == temporal_ref.LAST), t
        q += refresh == temporal_ref.LAST
    assert any(i[2] != temporal_ref.LAST and not i[3] for i in seen["infos"])


@pytest.mark.parametrize("w,h", [(64, 48), (176, 144)])
def test_a_forced_key_frame_restarts_the_phase(w, h):
    seen = run_driver((w, h, 1, "on", 0, (4,)), 1)
    assert [i[3] for i in seen["infos"]] == [t in (0, 4) for t in range(TOTAL)]
    assert [i[0] for i in seen["infos"]] == [0, 0, 1, 2, 0, 0, 1, 2]


@pytest.mark.parametrize("w,h", [(64, 48), (176, 144)])
def test_a_period_set_inside_a_gop_takes_force_at_the_next_frame_at_the_phase_the_gop_has_reached(w, h):
    seen = run_driver((w, h, 1, "from frame 3", 0, ()), 2)
    assert [i[1] > 0 for i in seen["infos"]] == [t >= 3 for t in range(TOTAL)]
    assert [i[0] for i in seen["infos"]] == [0] + list(range(TOTAL - 1))      # q advanced while refresh was off


def test_a_gop_coded_as_a_chunk_gives_the_serial_bytes():
    key = (64, 48, 1, "on", 0, (4,))
    serial = run_driver(key, 2)
    chunk = run_driver(key, 2, first=4, compare=False)      # a fresh driver, its first frame with force_key
    assert chunk["stream"] == serial["stream"][4:]
    for a, b in zip(chunk["recons"], serial["recons"][4:]):
        same(a, b, "chunk")


@pytest.mark.parametrize("layers", [1, 3])
def test_the_conformant_stream_decodes_to_the_device_reconstruction_and_heals_within_a_period(layers):
    """every decoded frame equals the device's reconstruction and the parsed intra set equals the rule's (run_driver); over P frames
    that refresh LAST the union of the intra sets is the whole picture"""
    w, h = 176, 144
    seen = run_driver((w, h, layers, "on", 1, ()), 2)
    sets = [s for s, i in zip(seen["intra"], seen["infos"]) if not i[3] and i[2] == temporal_ref.LAST]
    if layers == 1:
        assert len(sets) >= 4 and all(np.logical_or.reduce(sets[k:k + 4]).all() for k in range(len(sets) - 3))
        assert all(sum(s.astype(int) for s in sets[k:k + 4]).max() == 1 for k in range(len(sets) - 3))
    else:
        assert 0 < len(sets) < 4      # (eight frames of three layers hold one LAST-refreshing inter frame: no full sweep yet)


# ---- 3. off is off -----------------------------------------------------------------------------------------------------------------------------
def test_off_a_driver_launches_nothing_and_gives_the_bytes_it_gave():
    """a driver that never calls the setter, one with period 0, and one whose period was set and taken back before the first frame: the
    bytes and reconstructions of the oracle loop without the rule, and of the intra stage's launches only the key frame's"""
    from vp8oclenc_amd import api
    w, h = 64, 48
    frames = pan(w, h)
    key = (w, h, 1, "off", 0, ())
    streams = []
    for calls in ((), (0,), (4, 0)):
        drv = api.NativeDriver(w, h, gop_size=TOTAL, altref_range=TOTAL + 1, check_ssim=1, **QI)
        drv.hip.profile_enable(["intra"])
        for p in calls:
            drv.set_intra_refresh(p)
        out = []
        for t, f in enumerate(frames):
            drv.encode_frame_host(*f)
            out.append(drv.get_frame())
            drv.resolve()
            assert out[-1] == expected_bytes(key, t, 1), (calls, t)
            same(drv.hip.download_last(), oracle_records(*key)[t]["recon"], f"{calls} frame {t}")
            info = drv.intra_refresh()
            assert (info.period, info.last_forced, info.total_forced, info.last_q) == (0, 0, 0, max(0, t - 1)), (calls, t)
        assert drv.hip.profile_read()["intra"][1] == 1, calls      # the key frame's; with a period every inter frame adds one:
        drv.close()
        streams.append(out)
    assert streams[0] == streams[1] == streams[2]
    drv = api.NativeDriver(w, h, gop_size=TOTAL, altref_range=TOTAL + 1, check_ssim=1, **QI)
    drv.hip.profile_enable(["intra"])
    drv.set_intra_refresh(4)
    for f in frames:
        drv.encode_frame_host(*f)
        drv.resolve()
    assert drv.hip.profile_read()["intra"][1] == TOTAL
    drv.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_driver_and_nothing_has_changed():
    from vp8oclenc_amd import api, ref_shard
    w, h = 64, 48
    frames = pan(w, h)
    lib = api.load_library()
    lib.vp8drv_set_intra_refresh.argtypes = [C.c_void_p, C.c_int]
    lib.vp8drv_get_intra_refresh.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_shard_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    lib.vp8drv_encode_frame_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    good = dict(gop_size=TOTAL, altref_range=TOTAL + 1, check_ssim=1, **QI)
    key = (w, h, 1, "off", 0, ())

    def stream(drv, n=4):
        out = []
        for t in range(n):
            drv.encode_frame_host(*frames[t])
            out.append(drv.get_frame())
            drv.resolve()
        return out

    undisturbed = [expected_bytes(key, t, 1) for t in range(4)]
    drv = api.NativeDriver(w, h, **good)
    info = api.IntraRefreshInfo()
    assert lib.vp8drv_set_intra_refresh(None, 4) == ERR_ARG and lib.vp8drv_get_intra_refresh(None, C.byref(info)) == ERR_ARG
    assert lib.vp8drv_get_intra_refresh(drv.h, None) == ERR_ARG
    for period in (1, 2, 3, 1025, -1, -4):
        assert lib.vp8drv_set_intra_refresh(drv.h, period) == ERR_ARG, period
    # a member of a live batch; and a batch refuses a driver with a period
    other = api.NativeDriver(w, h, **good)
    batch = api.NativeBatch([drv, other])
    assert lib.vp8drv_set_intra_refresh(drv.h, 4) == ERR_STATE
    assert lib.vp8drv_set_intra_refresh(drv.h, 0) == 0      # (off is always accepted)
    batch.close()
    assert drv.intra_refresh().period == 0
    assert stream(drv) == undisturbed      # after all of them: an undisturbed driver's bytes
    drv.set_intra_refresh(8)
    for pair in ([drv, other], [other, drv]):
        with pytest.raises(api.Vp8HipError):
            api.NativeBatch(pair)
    other.close()
    drv.close()
    # the configuration: the host parameter mirror, an SSIM target above -1
    for cfg in (dict(good, device_params=0), dict(good, ssim_target=-0.5), dict(good, ssim_target=0.9)):
        d = api.NativeDriver(w, h, **cfg)
        for period in (4, 1024):
            assert lib.vp8drv_set_intra_refresh(d.h, period) == ERR_ARG, cfg
        assert lib.vp8drv_set_intra_refresh(d.h, 0) == 0 and d.intra_refresh().period == 0
        d.close()
    # a by-reference split: the setter, and -- joined behind the setter -- the calls that take a frame in
    drv = api.NativeDriver(w, h, **good)
    drv.set_intra_refresh(4)
    assert stream(drv, 1) == undisturbed[:1]
    last = [p.copy() for p in drv.hip.download_last()]
    assert lib.vp8hip_shard_init(drv.hip.h, ref_shard.shard_unique_id(), 0, 1) == 0
    y, u, v = (np.ascontiguousarray(p) for p in frames[1])
    assert lib.vp8drv_encode_frame_host(drv.h, y.ctypes.data, u.ctypes.data, v.ctypes.data, 0) == ERR_STATE
    assert lib.vp8drv_set_intra_refresh(drv.h, 8) == ERR_STATE and drv.intra_refresh().period == 4
    assert drv.stats().frame_number == 1
    same(drv.hip.download_last(), last, "LAST after the refusals")
    assert lib.vp8drv_set_intra_refresh(drv.h, 0) == 0
    drv.close()


def test_hidden_frames_carry_no_forced_macroblocks():
    """vp8drv_encode_arf_host between refreshed frames: the hidden frame parses as all inter, and the phase does not count it"""
    import vp8_parse as vp
    from vp8oclenc_amd import api
    w, h = 64, 48
    frames = pan(w, h)
    drv = api.NativeDriver(w, h, gop_size=TOTAL, altref_range=TOTAL + 1, check_ssim=1, **QI)
    drv.set_arf(4)
    drv.set_intra_refresh(4)
    st = vp.StreamState()
    qs = []
    for t in range(4):
        if t == 2:
            drv.encode_arf_host(frames[1:4], 1)
            f = vp.parse_frame(drv.get_frame(), st)
            assert not f.key and not f.show and (f.is_inter == 1).all()
        drv.encode_frame_host(*frames[t])
        f = vp.parse_frame(drv.get_frame(), st)
        drv.resolve()
        info = drv.intra_refresh()
        qs.append(info.last_q)
        if t:
            assert np.array_equal(f.is_inter == 0, ref.forced_map(w // 16, h // 16, 4, info.last_q).reshape(-1)), t
    assert qs == [0, 0, 1, 2]
    drv.close()
