"""Frame analysis statistics on the device (vp8hip_set_analysis: k_analyse_src_b behind every intake, k_analyse_mb_b behind every loop
filter) against the numpy restatement of tests/analysis_ref.py, field for field, whichever way a frame comes in, alone and in a batch,
beside the other opt-ins; vp8drv_set_quantizer against a driver created with the new pair; the tools' first-pass file.  Everything is
exact: no tolerances."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import analysis_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -4


def current_luma(hip):
    from vp8oclenc_amd import api
    return hip.debug(api.DBG_PYRAMID, 3, 0)


def source_of(rec):
    return {k: int(getattr(rec, k)) for k in ref.SOURCE_FIELDS}


def coding_of(rec):
    d = rec.as_dict()
    return {k: d[k] for k in ref.CODING_FIELDS}


def take(hip, frame, way, keep):
    """one frame into a context: by device pointers, from pageable host memory, or prefetched from page-locked memory"""
    from vp8oclenc_amd import api
    if way == "device":
        d = [api.to_device(p) for p in frame]
        hip.set_current_device(*[b.data_ptr() for b in d])
        hip.synchronize()
    elif way == "upload":
        hip.upload_current(*frame)
    else:
        hb = [api.HostBuffer(np.ascontiguousarray(p).ravel()) for p in frame]
        keep.append(hb)
        ptrs = [b.data_ptr() for b in hb]
        hip.lib.vp8hip_prefetch_current.argtypes = [C.c_void_p] * 4
        hip.lib.vp8hip_upload_current.argtypes = [C.c_void_p] * 4
        assert hip.lib.vp8hip_prefetch_current(hip.h, *ptrs) == 0
        assert hip.lib.vp8hip_upload_current(hip.h, *ptrs) == 0


# (coded size, source size or None): one macroblock (fewer lanes than a wave); two quads' worth of one row; rows of 176 and 80 bytes (no
# multiple of 64, the last quad of a row partly empty); a 40x24 source padded to 48x32 (the padding is measured)
GEOMETRIES = [((16, 16), None), ((48, 32), None), ((176, 144), None), ((48, 32), (40, 24)), ((80, 48), None)]


# ---- 1. the source side, context level --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coded,src", GEOMETRIES)
def test_source_side_equals_the_rule(coded, src):
    from vp8oclenc_amd import api
    W, H = coded
    w, h = src or coded
    hip = api.Vp8Hip(W, H)
    if src:
        hip.set_source_size(w, h)
    hip.set_analysis(True)
    frames = ref.video(w, h, 5, seed=W + h, still_from=1)      # frame 2 repeats frame 1: every macroblock static
    prev = None
    for t, f in enumerate(frames):
        if t == 3:
            hip.analysis_restart()
            prev = None
        hip.upload_current(*f)
        cur = current_luma(hip)
        assert cur.shape == (H, W)
        if src:
            assert np.array_equal(cur[:h, :w], f[0])
        r = hip.analysis_result()
        assert source_of(r) == ref.source_side(cur, prev), t
        assert (r.frame_number, r.coded, r.is_key, r.have_prev) == (t, 0, 0, int(t not in (0, 3)))
        assert all(v == 0 or v == [0] * len(v) for v in coding_of(r).values())      # not coded: the coding side is zero
        if t == 2:
            assert (r.static_mbs, r.temporal_sse, r.temporal_sad) == ((W // 16) * (H // 16), 0, 0)
        if t == 1:
            assert r.temporal_sad > 0 and r.spatial > 0
        prev = cur
    hip.close()


@pytest.mark.parametrize("way", ["device", "upload", "prefetch"])
def test_every_intake_path_of_a_context(way):
    from vp8oclenc_amd import api
    W, H = 48, 32
    hip = api.Vp8Hip(W, H)
    hip.set_analysis(True)
    keep, prev = [], None
    for t, f in enumerate(ref.video(W, H, 3, seed=3)):
        take(hip, f, way, keep)
        cur = current_luma(hip)
        assert np.array_equal(cur, f[0])
        r = hip.analysis_result()
        assert source_of(r) == ref.source_side(cur, prev) and r.frame_number == t, (way, t)
        prev = cur
    hip.close()


def test_off_means_state_errors_and_bad_arguments():
    from vp8oclenc_amd import api
    hip = api.Vp8Hip(48, 32)
    lib = hip.lib
    lib.vp8hip_analysis_result.argtypes = [C.c_void_p, C.c_void_p]
    lib.vp8hip_set_analysis.argtypes = [C.c_void_p, C.c_int]
    a = api.Analysis()
    assert lib.vp8hip_analysis_result(hip.h, C.byref(a)) == ERR_STATE      # off
    f = ref.video(48, 32, 2, seed=1)
    hip.upload_current(*f[0])
    hip.set_analysis(True)
    assert lib.vp8hip_analysis_result(hip.h, C.byref(a)) == ERR_STATE      # on, nothing taken in since
    assert lib.vp8hip_set_analysis(hip.h, 2) == ERR_ARG and lib.vp8hip_set_analysis(hip.h, -1) == ERR_ARG
    assert lib.vp8hip_analysis_result(hip.h, None) == ERR_ARG
    hip.upload_current(*f[1])
    assert hip.analysis_result().have_prev == 0                             # the frame taken in before it was on is no history
    hip.set_analysis(False)
    assert lib.vp8hip_analysis_result(hip.h, C.byref(a)) == ERR_STATE
    hip.close()


# ---- 2. the driver: every hand-over, both sides, fallback macroblocks and frames coded again ---------------------------------------
class Schedule:
    """the driver's GOP schedule mirrored: which incoming frames it makes key frames, given how the frames before ended"""

    def __init__(self, gop_size, altref_range):
        from vp8oclenc_amd import api
        self.g = api.Gop(gop_size, altref_range)

    def incoming_is_key(self):
        return bool(self.g.next().current_is_key)

    def done(self, ended_as_key):
        if ended_as_key:
            self.g.key_coded()
        self.g.frame_done()


def expected_coding_side(drv, ended_as_key, check_ran):
    """the rule on the arrays the driver's context holds for the frame just made final"""
    from vp8oclenc_amd import api
    res = drv.hip.download_results(recon=False)
    nz = drv.hip.debug(api.DBG_MB_NZ)
    flags = None
    replaced = drv.stats().last_replaced if (check_ran and not ended_as_key) else 0
    if replaced > 0:
        flags = drv.hip.download_intra()[1]
        assert int((flags == 0).sum()) == replaced
    return ref.coding_side(ended_as_key, res["MB_parts"], res["MB_reference_frame"], res["MB_vectors"], nz, res["MB_segment_id"], flags), replaced


def run_driver(frames, way, **cfg):
    """-> per frame (record, ended as key, replaced), every record held against both rules on the way"""
    from vp8oclenc_amd import api
    W, H = frames[0][0].shape[1], frames[0][0].shape[0]
    cfg = dict(dict(gop_size=4, altref_range=2, check_ssim=1, num_partitions=1), **cfg)
    drv = api.NativeDriver(W, H, **cfg)
    drv.set_analysis(True)
    sched = Schedule(cfg["gop_size"], cfg["altref_range"])
    ny, nc = W * H, (W // 2) * (H // 2)
    host = [api.HostBuffer(np.concatenate([p.ravel() for p in f])) for f in frames]
    ptrs = [(hb.data_ptr(), hb.data_ptr() + ny, hb.data_ptr() + ny + nc) for hb in host]
    drv.lib.vp8drv_stage_frame_host.argtypes = [C.c_void_p] * 4
    out, prev = [], None
    for t, f in enumerate(frames):
        if sched.incoming_is_key():
            prev = None
        if way == "device":
            dev = [api.to_device(p) for p in f]
            key = drv.encode_frame_device(*[x.data_ptr() for x in dev])
        elif way == "host":
            key = drv.encode_frame_host(*f)
        elif way == "prefetch":
            if t == 0:
                drv.prefetch_frame_host_ptr(*ptrs[0])
            key = drv.encode_frame_host_ptr(*ptrs[t])
            if t + 1 < len(frames):
                drv.prefetch_frame_host_ptr(*ptrs[t + 1])
        else:      # stage: frame t was handed over early behind frame t - 1, below
            key = drv.encode_frame_host_ptr(*ptrs[t])
        ended_as_key = drv.resolve() or key
        cur = current_luma(drv.hip)
        want_coding, replaced = expected_coding_side(drv, ended_as_key, bool(cfg["check_ssim"]))
        drv.get_frame()
        if way == "stage" and t + 1 < len(frames):      # the NEXT frame becomes current before this frame's record is read
            assert drv.lib.vp8drv_stage_frame_host(drv.h, *ptrs[t + 1]) == 0
        r = drv.frame_analysis()
        assert (r.frame_number, r.coded, r.is_key) == (t, 1, int(ended_as_key)), (way, t)
        assert source_of(r) == ref.source_side(cur, prev), (way, t)
        assert coding_of(r) == want_coding, (way, t)
        mbs = (W // 16) * (H // 16)
        assert r.mbs_intra + sum(r.mbs_ref) == mbs == sum(r.segment_mbs) == r.mbs_total
        out.append((r.as_dict(), ended_as_key, replaced))
        sched.done(ended_as_key)
        prev = cur
    drv.close()
    return out


@pytest.mark.parametrize("way", ["device", "host", "prefetch", "stage"])
def test_driver_records_whichever_way_the_frames_come_in(way):
    W, H = 48, 32
    out = run_driver(ref.video(W, H, 6, seed=11), way)
    assert [r["have_prev"] for r, _, _ in out][0] == 0
    assert any(r["have_prev"] == 0 for r, _, _ in out[1:])      # the schedule's second GOP restarted the history
    assert any(not k and r["mbs_ref"][0] > 0 for r, k, _ in out)
    assert out[0][1] and out[0][0]["mbs_intra"] == 6


def test_coding_side_with_fallback_macroblocks_and_frames_coded_again():
    """coarse quantizers, an SSIM target of 0.90 and a scene cut on an ordinary inter frame (the sequence of tests/test_gpu_intra.py): inter
    frames keep fallback macroblocks (the flags count) and the cut frame is sent back and coded again as a key frame (the key frame's
    record, the source side measured once)"""
    from vp8oclenc_amd.synth import SynthSequence
    W, H = 320, 192
    a_seq, b_seq = SynthSequence(W, H, seed=41), SynthSequence(W, H, seed=97)
    frames = [a_seq.frame(t) for t in range(4)] + [b_seq.frame(t) for t in range(4)]
    out = run_driver(frames, "host", gop_size=150, altref_range=5, qi_min=50, qi_max=110, ssim_target=0.90)
    kept_fallback = [t for t, (r, k, repl) in enumerate(out) if not k and repl > 0]
    sent_back = [t for t, (r, k, repl) in enumerate(out) if k and t > 0]
    print(f"inter frames that kept fallback macroblocks: {kept_fallback}, frames coded again as key frames: {sent_back}")
    assert kept_fallback, "no inter frame kept a fallback macroblock: the case does not count"
    assert sent_back, "no frame was sent back and coded again as a key frame"
    for t in kept_fallback:
        assert out[t][0]["mbs_intra"] == out[t][2] and out[t][0]["is_key"] == 0
    for t in sent_back:      # the key frame's coding side, the history not restarted (the schedule did not start a GOP there)
        assert out[t][0]["mbs_intra"] == (W // 16) * (H // 16) and out[t][0]["mbs_ref"] == [0, 0, 0] and out[t][0]["have_prev"] == 1


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------
def test_batch_members_give_the_records_they_give_alone():
    from vp8oclenc_amd import api
    W, H = 48, 32
    vids = [ref.video(W, H, 5, seed=21), ref.video(W, H, 5, seed=22)]
    cfg = dict(gop_size=3, altref_range=2, check_ssim=1, num_partitions=1)
    alone = []
    for v in vids:
        d = api.NativeDriver(W, H, **cfg)
        d.set_analysis(True)
        recs = []
        for f in v:
            d.encode_frame_host(*f)
            recs.append(d.frame_analysis().as_dict())
            d.get_frame()
        alone.append(recs)
        d.close()
    drvs = [api.NativeDriver(W, H, **cfg) for _ in vids]
    drvs[0].set_analysis(True)
    with pytest.raises(api.Vp8HipError):      # members that differ in the setting are refused
        api.NativeBatch(drvs)
    lib = drvs[0].lib
    lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
    hb = C.c_void_p()
    ctxs = (C.c_void_p * 2)(drvs[0].hip.h.value, drvs[1].hip.h.value)
    assert lib.vp8hip_batch_create(C.byref(hb), ctxs, 2) == ERR_ARG      # ... at the context level too
    drvs[1].set_analysis(True)
    b = api.NativeBatch(drvs)
    lib.vp8drv_set_analysis.argtypes = [C.c_void_p, C.c_int]
    lib.vp8drv_set_quantizer.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert lib.vp8drv_set_analysis(drvs[0].h, 0) == ERR_STATE            # a live batch member
    assert lib.vp8drv_set_quantizer(drvs[0].h, 10, 50) == ERR_STATE
    for t in range(5):
        dev = [[api.to_device(p) for p in v[t]] for v in vids]
        b.encode_frame_device([tuple(x.data_ptr() for x in d) for d in dev])
        for i, d in enumerate(drvs):
            assert d.frame_analysis().as_dict() == alone[i][t], (i, t)
        b.get_frames_begin()
        for d in drvs:
            d.get_frame_end()
    b.close()
    assert lib.vp8drv_set_analysis(drvs[0].h, 0) == 0                    # the batch is gone
    for d in drvs:
        d.close()


def test_batched_upload_takes_the_frames_too():
    from vp8oclenc_amd import api
    W, H = 48, 32
    vids = [ref.video(W, H, 3, seed=31), ref.video(W, H, 3, seed=32)]
    drvs = [api.NativeDriver(W, H, gop_size=1 << 20, check_ssim=1) for _ in vids]
    for d in drvs:
        d.set_analysis(True)
    b = api.NativeBatch(drvs)
    ny, nc = W * H, (W // 2) * (H // 2)
    host = [[api.HostBuffer(np.concatenate([p.ravel() for p in f])) for f in v] for v in vids]
    prev = [None, None]
    for t in range(3):
        b.encode_frame_host([(hb[t].data_ptr(), hb[t].data_ptr() + ny, hb[t].data_ptr() + ny + nc) for hb in host])
        for i, d in enumerate(drvs):
            r = d.frame_analysis()
            cur = vids[i][t][0]
            assert source_of(r) == ref.source_side(cur, prev[i]) and r.coded == 1, (i, t)
            prev[i] = cur
        b.get_frames_begin()
        for d in drvs:
            d.get_frame_end()
    b.close()
    for d in drvs:
        d.close()


# ---- 4. off means off --------------------------------------------------------------------------------------------------------------
def test_the_bytes_do_not_change():
    from vp8oclenc_amd import api
    W, H = 48, 32
    frames = ref.video(W, H, 5, seed=41)
    cfg = dict(gop_size=4, altref_range=2, check_ssim=1, num_partitions=2)
    off, on = api.NativeDriver(W, H, **cfg), api.NativeDriver(W, H, **cfg)
    on.set_analysis(True)
    a = api.Analysis()
    off.lib.vp8drv_get_frame_analysis.argtypes = [C.c_void_p, C.c_void_p]
    assert off.lib.vp8drv_get_frame_analysis(on.h, C.byref(a)) == ERR_STATE      # on, no frame yet
    for t, f in enumerate(frames):
        off.encode_frame_host(*f)
        on.encode_frame_host(*f)
        assert off.get_frame() == on.get_frame(), t
        assert off.lib.vp8drv_get_frame_analysis(off.h, C.byref(a)) == ERR_STATE      # never turned on
        assert on.frame_analysis().frame_number == t
    off.close()
    on.close()


# ---- 5. beside the other opt-ins ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["denoise", "nv12"])
def test_the_frame_measured_is_the_frame_that_is_coded(what):
    from vp8oclenc_amd import api
    W, H = 48, 32
    hip = api.Vp8Hip(W, H)
    if what == "denoise":
        hip.set_denoise(1)
    else:
        hip.set_source_format(api.FORMAT_NV12)
    hip.set_analysis(True)
    prev, changed = None, False
    # (a still picture under fresh noise for the denoiser: a picture that drifts is left alone by its block decision)
    for t, f in enumerate(ref.noisy_still(W, H, 4, seed=51) if what == "denoise" else ref.video(W, H, 4, seed=51)):
        if what == "nv12":
            p = api.planes_from_i420(api.FORMAT_NV12, *f)
            hip.upload_current(p[0], p[1], p[1])
        else:
            hip.upload_current(*f)
        cur = current_luma(hip)
        changed = changed or not np.array_equal(cur, f[0])
        assert source_of(hip.analysis_result()) == ref.source_side(cur, prev), (what, t)
        prev = cur
    assert changed == (what == "denoise")      # (the denoiser did change frames: what was measured is its output)
    hip.close()


# ---- 6. the quantizer setter -------------------------------------------------------------------------------------------------------
def test_set_quantizer_behind_a_key_frame_is_a_driver_created_with_the_pair():
    from vp8oclenc_amd import api
    W, H = 48, 32
    frames = ref.video(W, H, 6, seed=61)
    cfg = dict(gop_size=3, altref_range=2, check_ssim=1, num_partitions=1)
    a, plain, b = api.NativeDriver(W, H, qi_min=0, qi_max=48, **cfg), api.NativeDriver(W, H, qi_min=0, qi_max=48, **cfg), \
        api.NativeDriver(W, H, qi_min=20, qi_max=60, **cfg)
    assert a.quantizer() == (0, 48) and b.quantizer() == (20, 60)
    out_a, out_plain = [], []
    for t, f in enumerate(frames):
        if t == 3:
            a.set_quantizer(20, 60)
            assert a.quantizer() == (20, 60)
        a.encode_frame_host(*f)
        plain.encode_frame_host(*f)
        out_a.append(a.get_frame())
        out_plain.append(plain.get_frame())
    out_b = []
    for f in frames[3:]:
        b.encode_frame_host(*f)
        out_b.append(b.get_frame())
    assert out_a[:3] == out_plain[:3]
    assert out_a[3] != out_plain[3]                 # the setter is no no-op
    assert out_a[3:] == out_b                       # a closed GOP is self-contained: nothing but the references outlives a key frame
    lib = a.lib
    lib.vp8drv_set_quantizer.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.vp8drv_get_quantizer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for bad in ((-1, 48), (0, 128), (200, 10), (0, -5)):
        assert lib.vp8drv_set_quantizer(a.h, *bad) == ERR_ARG
    assert a.quantizer() == (20, 60)                # a refused pair changed nothing
    q = C.c_int32()
    assert lib.vp8drv_get_quantizer(a.h, None, C.byref(q)) == ERR_ARG and lib.vp8drv_get_quantizer(None, C.byref(q), C.byref(q)) == ERR_ARG
    a.set_quantizer(60, 20)                         # as vp8drv_create: given as they are, used in order
    assert a.quantizer() == (60, 20)
    for d in (a, plain, b):
        d.close()


# ---- 7. the tools ------------------------------------------------------------------------------------------------------------------
def test_y4m_to_ivf_writes_the_first_pass_file(tmp_path):
    from vp8oclenc_amd import api, y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "y4m_to_ivf")
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", "y4m_to_ivf.cpp"), "-o", exe,
                    "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    W, H = 48, 32
    frames = ref.video(W, H, 3, seed=71)
    y4m.write_y4m(str(tmp_path / "in.y4m"), frames, framerate=25)
    common = [str(tmp_path / "in.y4m")]
    for out, extra in (("plain.ivf", []), ("an.ivf", ["-analysis", str(tmp_path / "pass1.txt")])):
        r = subprocess.run([exe, common[0], str(tmp_path / out), "-g", "30"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "plain.ivf", "rb").read() == open(tmp_path / "an.ivf", "rb").read()
    lines = open(tmp_path / "pass1.txt").read().splitlines()
    assert len(lines) == 3
    drv = api.NativeDriver(W, H, gop_size=30, scene_detect=1)
    drv.set_analysis(True)
    for t, f in enumerate(frames):
        drv.encode_frame_host(*f)
        rec = drv.frame_analysis()
        assert lines[t] == rec.text_line(len(drv.get_frame())), t
    drv.close()
    # scripts/encode_ivf.py --analysis: the same lines and the same file, with a GOP that ends inside the three frames (two chunks, each
    # on a driver of its own: the frame numbers are the file's, the history restarts where the serial program's schedule restarts it)
    import sys
    for out, extra in (("g2.ivf", ["-g", "2", "-no-scene-detect", "-analysis", str(tmp_path / "g2.txt")]),):
        r = subprocess.run([exe, common[0], str(tmp_path / out)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "py.ivf"), "--y4m", common[0], "--frames", "3", "--gop", "2",
                        "--analysis", str(tmp_path / "py.txt")], capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "py.ivf", "rb").read() == open(tmp_path / "g2.ivf", "rb").read()
    g2 = open(tmp_path / "g2.txt").read().splitlines()
    assert open(tmp_path / "py.txt").read().splitlines() == g2 and len(g2) == 3
    assert [int(line.split()[3]) for line in g2] == [0, 1, 0]      # have_prev: frame 2 starts the second GOP
