"""A batched call that REFUSES (vp8hip_batch_*: every member is checked before any member's state changes) leaves the batch as it found
it: the call returns VP8HIP_ERR_STATE, the other two members, driven on with the offender sitting out, give what two contexts on
their own give for the same frames, byte for byte, and so does the offender once it has been made valid.

Three members of 64x48 (4 x 3 macroblocks), each on its own rotation of the four frames of tests/golden/g64x48_last_only.npz; the
contexts on their own are coded once per flow (alone()) and shared by the cases."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 3
ERR_STATE = -4      # VP8HIP_ERR_STATE, include/vp8hip.h
TARGET = 0.90       # the cases with check_SSIM (the others: -1, the reference's default)
REFQI, QI_MIN = (20, 30, 40, 50), 4
PARTITIONS = 2
RESULT_KEYS = ("MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs", "MB_segment_id", "MB_SSIM", "prefilter_Y", "prefilter_U", "prefilter_V")


class HeaderParams(C.Structure):      # vp8hip_header_params
    _fields_ = [(n, C.c_int32) for n in ("is_key", "is_golden", "is_altref", "loop_filter_type", "loop_filter_sharpness", "partitions_log2",
                                          "width", "height", "use_intra_info")]


INTER_HEADER = dict(is_key=0, is_golden=0, is_altref=0, loop_filter_type=0, loop_filter_sharpness=0, partitions_log2=1, width=0, height=0,
                    use_intra_info=0)


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g64x48_last_only.npz"))
    pool = [tuple(np.ascontiguousarray(g[f"in_{name}_{p}"]) for p in "YUV") for name in ("ref0", "cur", "ref1", "ref2")]
    assert len(set(f[0].tobytes() for f in pool)) == 4
    return pool, np.ascontiguousarray(g["segments"], np.int32)


def frame(i, t):
    """frame t of member i: every member has its own content at every t"""
    return _golden()[0][(i + t) % 4]


def _lib():
    lib = api.load_library()
    ints, vp = C.POINTER(C.c_int), C.c_void_p
    lib.vp8hip_batch_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int]
    lib.vp8hip_batch_destroy.argtypes = [vp]
    lib.vp8hip_batch_destroy.restype = None
    lib.vp8hip_batch_inter_transform.argtypes = [vp] + [ints] * 5
    lib.vp8hip_batch_loop_filter.argtypes = [vp, ints]
    lib.vp8hip_batch_auto_segments.argtypes = [vp, ints, ints, C.POINTER(C.c_int32 * 4), C.c_int]
    lib.vp8hip_batch_check_ssim_async.argtypes = [vp, ints, C.POINTER(C.c_int32 * 4), C.c_int]
    lib.vp8hip_batch_encode_frame_begin.argtypes = [vp, ints, C.c_int, C.POINTER(HeaderParams)]
    lib.vp8hip_encode_frame_begin.argtypes = [vp, C.c_int, C.POINTER(HeaderParams)]
    lib.vp8hip_encode_frame_end.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    return lib


def new_context(target):
    c = api.Vp8Hip(W, H, target)
    c.set_segments(_golden()[1])
    return c


def key_frame(c, i):
    """frame 0 of member i as a key frame, filtered: the context has a LAST and nothing else"""
    c.upload_current(*frame(i, 0))
    c.intra_transform()
    c.prepare_filter_mask(want_nz=False)
    c.loop_filter()


def frame_bytes_begin(c):
    assert c.lib.vp8hip_encode_frame_begin(c.h, PARTITIONS, C.byref(HeaderParams(**INTER_HEADER))) == 0


def frame_bytes_end(c):
    out, n = np.zeros(c.mbs * 1024 + 16384, np.uint8), C.c_size_t(0)
    assert c.lib.vp8hip_encode_frame_end(c.h, out.ctypes.data, out.size, C.byref(n)) == 0
    return out[:n.value].tobytes()


@functools.lru_cache(maxsize=None)
def alone(i, golden=False, check=False, frames=1, coded=False, scan=False):
    """Member i's frames 1 .. `frames` on a context of its own, behind its key frame: per frame what the inter transform left
    (download_results), check_SSIM's verdict, the filtered frame (download_last) and the coded bytes.  golden: GOLDEN := LAST, and used.
    scan: the frame's segment data come from the parameter scan (vp8hip_auto_segments) and are part of what is compared."""
    _lib()
    c = new_context(TARGET if check else -1.0)
    try:
        key_frame(c, i)
        out = []
        for t in range(1, frames + 1):
            c.upload_current(*frame(i, t))
            if scan:
                c.auto_segments(False, REFQI, QI_MIN)
            c.inter_transform(1 if golden else 0, 0, 1 if golden else 0, 0)
            if check:
                c.check_ssim_async(REFQI, QI_MIN)
            r = dict(results=c.download_results(recon=True))
            if scan:
                r["segments"] = segments(c)
            c.loop_filter()
            if check:
                r["verdict"] = verdict(c)
            r["last"] = c.download_last()
            if coded:
                frame_bytes_begin(c)
                r["bytes"] = frame_bytes_end(c)
            out.append(r)
        return out
    finally:
        c.close()


def verdict(c):
    """check_SSIM's verdict, the two floats by their bits"""
    replaced, new_ssim, min_ssim, updated = c.check_ssim_result()
    return replaced, np.float32(new_ssim).tobytes(), np.float32(min_ssim).tobytes(), updated


def segments(c):
    """the segment data in force and the strength pair beside them"""
    sd, reductor, sharpness = c.get_segments()
    return np.asarray(sd).tobytes(), int(reductor), int(sharpness)


def same_results(c, want, what):
    if "segments" in want:
        assert segments(c) == want["segments"], f"{what}: the segment data differ from the context on its own"
    got = c.download_results(recon=True)
    for k in RESULT_KEYS:
        assert got[k].tobytes() == want["results"][k].tobytes(), f"{what}: {k} differs from the context on its own"


def same_last(c, want, what):
    for p, q in zip(c.download_last(), want["last"]):
        assert p.tobytes() == q.tobytes(), f"{what}: the filtered frame differs from the context on its own"


class Batch:
    """three contexts in a batch; the batched entry points by their return code, `on` = the members that take part (None: all)"""

    def __init__(self, target=-1.0, keyed=(0, 1, 2)):
        self.lib = _lib()
        self.m = [new_context(target) for _ in range(N)]
        self.hb = C.c_void_p()
        assert self.lib.vp8hip_batch_create(C.byref(self.hb), (C.c_void_p * N)(*[c.h for c in self.m]), N) == 0
        for i in keyed:
            key_frame(self.m[i], i)

    def close(self):
        if self.hb:
            self.lib.vp8hip_batch_destroy(self.hb)
            self.hb = None
        for c in self.m:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _on(on):
        return None if on is None else (C.c_int * N)(*[1 if i in on else 0 for i in range(N)])

    def current(self, t, members=(0, 1, 2)):
        for i in members:
            self.m[i].upload_current(*frame(i, t))

    def inter_transform(self, on=None, prev_is_golden=(0, 0, 0), use_golden=(0, 0, 0)):
        ints = lambda v: (C.c_int * N)(*v)
        return self.lib.vp8hip_batch_inter_transform(self.hb, self._on(on), ints(prev_is_golden), ints([0] * N), ints(use_golden), ints([0] * N))

    def auto_segments(self, on=None):
        q = ((C.c_int32 * 4) * N)(*[(C.c_int32 * 4)(*REFQI) for _ in range(N)])
        return self.lib.vp8hip_batch_auto_segments(self.hb, self._on(on), (C.c_int * N)(*([0] * N)), q, QI_MIN)

    def loop_filter(self, on=None):
        return self.lib.vp8hip_batch_loop_filter(self.hb, self._on(on))

    def check_ssim_async(self, on=None):
        q = ((C.c_int32 * 4) * N)(*[(C.c_int32 * 4)(*REFQI) for _ in range(N)])
        return self.lib.vp8hip_batch_check_ssim_async(self.hb, self._on(on), q, QI_MIN)

    def encode_frame_begin(self, on=None):
        p = (HeaderParams * N)(*[HeaderParams(**INTER_HEADER) for _ in range(N)])
        return self.lib.vp8hip_batch_encode_frame_begin(self.hb, self._on(on), PARTITIONS, p)


OTHERS, OFFENDER = (0, 2), 1


@pytest.mark.parametrize("case", ["no_last", "no_golden"])
def test_inter_transform_refuses_and_changes_nothing(case):
    with Batch(keyed=OTHERS if case == "no_last" else (0, 1, 2)) as b:
        b.current(1)
        use_golden = (0, 1, 0) if case == "no_golden" else (0, 0, 0)      # (no member has a GOLDEN: only the middle one asks for it)
        assert b.inter_transform(None, use_golden=use_golden) == ERR_STATE
        assert b.inter_transform(OTHERS, use_golden=use_golden) == 0
        for i in OTHERS:
            same_results(b.m[i], alone(i)[0], f"member {i}")
        assert b.loop_filter(OTHERS) == 0
        for i in OTHERS:
            same_last(b.m[i], alone(i)[0], f"member {i}")
        # the offender, made valid: its key frame first / GOLDEN := LAST in the same call
        if case == "no_last":
            key_frame(b.m[OFFENDER], OFFENDER)
            b.current(1, (OFFENDER,))
            want = alone(OFFENDER)[0]
            assert b.inter_transform((OFFENDER,)) == 0
        else:
            want = alone(OFFENDER, golden=True)[0]
            assert b.inter_transform((OFFENDER,), prev_is_golden=(0, 1, 0), use_golden=(0, 1, 0)) == 0
        same_results(b.m[OFFENDER], want, "the offender")
        assert b.loop_filter((OFFENDER,)) == 0
        same_last(b.m[OFFENDER], want, "the offender")


def test_auto_segments_refuses_and_changes_nothing():
    """the middle member has never been given a frame: nobody's parameter blocks trade places, nobody's scan is asked for"""
    with Batch(keyed=OTHERS) as b:
        b.current(1, OTHERS)
        assert b.auto_segments(None) == ERR_STATE
        assert b.auto_segments(OTHERS) == 0
        assert b.inter_transform(OTHERS) == 0
        for i in OTHERS:
            same_results(b.m[i], alone(i, scan=True)[0], f"member {i}")
        assert b.loop_filter(OTHERS) == 0
        for i in OTHERS:
            same_last(b.m[i], alone(i, scan=True)[0], f"member {i}")
        key_frame(b.m[OFFENDER], OFFENDER)
        b.current(1, (OFFENDER,))
        want = alone(OFFENDER, scan=True)[0]
        assert b.auto_segments((OFFENDER,)) == 0
        assert b.inter_transform((OFFENDER,)) == 0
        same_results(b.m[OFFENDER], want, "the offender")
        assert b.loop_filter((OFFENDER,)) == 0
        same_last(b.m[OFFENDER], want, "the offender")


@pytest.mark.parametrize("case", ["no_reconstruction", "filter_types_disagree"])
def test_loop_filter_refuses_and_changes_nothing(case):
    with Batch() as b:
        b.current(1)
        if case == "no_reconstruction":
            assert b.inter_transform(OTHERS) == 0
        else:
            assert b.inter_transform(None) == 0
            b.m[OFFENDER].set_loop_filter_type(1)
        assert b.loop_filter(None) == ERR_STATE
        for i in OTHERS:      # (the refused call has neither filtered nor released their reconstructions)
            same_results(b.m[i], alone(i)[0], f"member {i}")
        assert b.loop_filter(OTHERS) == 0
        for i in OTHERS:
            same_last(b.m[i], alone(i)[0], f"member {i}")
        if case == "no_reconstruction":
            assert b.inter_transform((OFFENDER,)) == 0
        else:
            b.m[OFFENDER].set_loop_filter_type(0)
        same_results(b.m[OFFENDER], alone(OFFENDER)[0], "the offender")
        assert b.loop_filter((OFFENDER,)) == 0
        same_last(b.m[OFFENDER], alone(OFFENDER)[0], "the offender")


def test_check_ssim_async_refuses_and_changes_nothing():
    with Batch(target=TARGET) as b:
        b.current(1)
        assert b.inter_transform(None) == 0
        b.m[OFFENDER].check_ssim_async(REFQI, QI_MIN)      # armed by its own entry point
        assert b.check_ssim_async(None) == ERR_STATE
        assert b.check_ssim_async(OTHERS) == 0
        for i in OTHERS:
            same_results(b.m[i], alone(i, check=True)[0], f"member {i}")
        assert b.loop_filter(OTHERS) == 0
        for i in OTHERS:
            assert verdict(b.m[i]) == alone(i, check=True)[0]["verdict"], f"member {i}"
            same_last(b.m[i], alone(i, check=True)[0], f"member {i}")
        # the offender's own check is a valid one: it rides in the filter launch of the offender
        want = alone(OFFENDER, check=True)[0]
        same_results(b.m[OFFENDER], want, "the offender")
        assert b.loop_filter((OFFENDER,)) == 0
        assert verdict(b.m[OFFENDER]) == want["verdict"]
        same_last(b.m[OFFENDER], want, "the offender")


def test_encode_frame_begin_refuses_and_changes_nothing():
    with Batch() as b:
        b.current(1)
        assert b.inter_transform(None) == 0
        assert b.loop_filter(None) == 0
        frame_bytes_begin(b.m[OFFENDER])      # pending, by its own entry point
        assert b.encode_frame_begin(None) == ERR_STATE
        assert b.encode_frame_begin(OTHERS) == 0
        for i in OTHERS:
            want = alone(i, coded=True)[0]
            assert frame_bytes_end(b.m[i]) == want["bytes"], f"member {i}: the coded frame differs from the context on its own"
            same_last(b.m[i], want, f"member {i}")
        # the offender's pending frame is a valid one; its next frame goes through the batch
        want = alone(OFFENDER, frames=2, coded=True)
        assert frame_bytes_end(b.m[OFFENDER]) == want[0]["bytes"]
        same_last(b.m[OFFENDER], want[0], "the offender")
        b.current(2, (OFFENDER,))
        assert b.inter_transform((OFFENDER,)) == 0
        same_results(b.m[OFFENDER], want[1], "the offender, next frame")
        assert b.loop_filter((OFFENDER,)) == 0
        assert b.encode_frame_begin((OFFENDER,)) == 0
        assert frame_bytes_end(b.m[OFFENDER]) == want[1]["bytes"]
        same_last(b.m[OFFENDER], want[1], "the offender, next frame")
