"""The deinterlacer's contract without a GPU: the numpy restatement of include/vp8hip_host.h's rule (tests/deinterlace_ref.py) against
vp8host_deinterlace_frame byte for byte, the properties the rule promises, its worth on a moving scene, the Y4M header's I tag
(vp8host_y4m_interlace) beside the reference's parser, and the ABI: new entry points, vp8drv_config and the ABI version unchanged.
tests/test_gpu_deinterlace.py holds the kernel to the same restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deinterlace_ref as ref
from vp8oclenc_amd import api, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (2, 4), (50, 36), (56, 40), (128, 96)]      # (50, 36): chroma 25 x 18, an odd width
MODES = [1, 2]
KEEPS = [0, 1]
NEW_SYMBOLS = ["vp8hip_set_deinterlace", "vp8hip_deinterlace_restart", "vp8hip_deinterlace_result", "vp8host_deinterlace_frame",
               "vp8host_y4m_interlace", "vp8drv_set_deinterlace", "vp8drv_get_deinterlace_stats"]


def _run_host(frames, mode, keep, restart_at=()):
    """the sequence through vp8host_deinterlace_frame -> list of (out, woven)"""
    hist = [np.zeros_like(p) for p in frames[0]] if mode == 2 else None
    have, res = False, []
    for t, f in enumerate(frames):
        if t in restart_at:
            have = False
        res.append(api.deinterlace_frame(f, hist, mode, keep, have))
        have = mode == 2
        if mode == 2:
            for a, b in zip(hist, f):
                assert np.array_equal(a, b)      # the frame as received is the new history
    return res


def _run_ref(frames, mode, keep, restart_at=()):
    d, res = ref.Deinterlacer(mode, keep), []
    for t, f in enumerate(frames):
        if t in restart_at:
            d.restart()
        res.append(d.take(f))
    return res


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", SIZES)
def test_host_function_equals_the_restatement_byte_for_byte(w, h, mode, keep):
    for name, frames in ref.sequences(w, h, seed=w + 3 * mode + keep).items():
        got, want = _run_host(frames, mode, keep, restart_at=(3,)), _run_ref(frames, mode, keep, restart_at=(3,))
        for t, ((go, gn), (wo, wn, missing)) in enumerate(zip(got, want)):
            for p in range(3):
                assert np.array_equal(go[p], wo[p]), (name, t, p)
            assert gn == wn and missing == w * h // 2, (name, t)
        if mode == 2 and name != "moving" and w > 2:
            assert any(n > 0 for _, n in got)      # (something was woven: the test is not about the field interpolation alone)


@pytest.mark.parametrize("keep", KEEPS)
def test_kept_rows_are_untouched_and_outputs_lie_between_s_and_wv(keep):
    for w, h in SIZES:
        for name, frames in ref.sequences(w, h, seed=11).items():
            for mode in MODES:
                for (out, _), f in zip(_run_host(frames, mode, keep), frames):
                    for p in range(3):
                        assert np.array_equal(out[p][keep::2], f[p][keep::2]), (name, mode, p)
                        s, wv, o = ref.spatial(f[p], keep)[1 - keep::2], f[p][1 - keep::2].astype(int), out[p][1 - keep::2].astype(int)
                        assert ((o >= np.minimum(s, wv)) & (o <= np.maximum(s, wv))).all(), (name, mode, p)
                        if mode == 1:
                            assert np.array_equal(o, s)


@pytest.mark.parametrize("keep", KEEPS)
def test_mode_2_without_a_history_is_mode_1(keep):
    for w, h in SIZES:
        frames = ref.sequences(w, h, seed=5)["moving"]
        one = _run_host(frames, 1, keep)
        two = _run_host(frames, 2, keep, restart_at=range(len(frames)))      # restarted in front of every frame
        for (a, na), (b, nb) in zip(one, two):
            assert na == nb == 0 and all(np.array_equal(p, q) for p, q in zip(a, b))
        later = _run_host(frames, 2, keep)
        assert all(np.array_equal(p, q) for p, q in zip(one[0][0], later[0][0]))      # the first frame
        if w > 2:
            assert any(not np.array_equal(one[t][0][0], later[t][0][0]) for t in range(1, len(frames)))      # (and on is on)


@pytest.mark.parametrize("keep", KEEPS)
def test_a_static_sequence_comes_back_exactly(keep):
    for w, h in SIZES:
        frames = ref.sequences(w, h, seed=8)["static"]
        res = _run_host(frames, 2, keep)
        assert res[0][1] == 0
        for (out, woven), f in list(zip(res, frames))[1:]:
            assert woven == w * h // 2
            assert all(np.array_equal(p, q) for p, q in zip(out, f))


@pytest.mark.parametrize("keep", KEEPS)
def test_a_plane_linear_in_y_is_reproduced_by_mode_1(keep):
    w, h = 16, 40
    y = np.repeat((20 + 5 * np.arange(h))[:, None], w, axis=1).astype(np.uint8)
    c = np.repeat((30 + 7 * np.arange(h // 2))[:, None], w // 2, axis=1).astype(np.uint8)
    out, _ = api.deinterlace_frame([y, c, c], None, 1, keep, False)
    for o, p in zip(out, (y, c, c)):
        # kept rows v - d, v, v + d, v + 2 d around a missing row: (16 v + 8 d + 8) >> 4 = v + d / 2 for an even d, and d is twice the slope
        inner = slice(6, p.shape[0] - 6)      # every tap of these rows is a row of its own: nothing is clamped
        assert np.array_equal(o[inner], p[inner])
        assert not np.array_equal(o, p)       # (at the ends the clamped taps bend the line)


@pytest.mark.parametrize("keep", KEEPS)
def test_adaptive_beats_field_and_untouched_on_a_moving_scene(keep):
    w, h = 64, 48
    d1, d2 = ref.Deinterlacer(1, keep), ref.Deinterlacer(2, keep)
    for t in range(6):
        inter, prog = ref.moving_scene(w, h, t, keep)
        o1, o2 = d1.take(inter)[0][0], d2.take(inter)[0][0]
        if t == 0:
            continue
        sse = lambda a: float(((a.astype(np.int64) - prog[0].astype(np.int64)) ** 2).sum())
        e_raw, e1, e2 = sse(inter[0]), sse(o1), sse(o2)
        psnr = lambda e: 10 * np.log10(255.0 ** 2 * w * h / e)
        print(f"keep {keep} frame {t}: untouched {psnr(e_raw):.2f} dB, field {psnr(e1):.2f} dB, adaptive {psnr(e2):.2f} dB")
        assert e2 < e1 and e2 < e_raw, (t, e_raw, e1, e2)


HEAD = b"YUV4MPEG2 W34 H18 F25:1 "
TAGS = [(None, api.FIELDS_PROGRESSIVE), (b"Ip", api.FIELDS_PROGRESSIVE), (b"I?", api.FIELDS_PROGRESSIVE), (b"It", api.FIELDS_TOP_FIRST),
        (b"Ib", api.FIELDS_BOTTOM_FIRST), (b"Im", -1)]


def _headers(tag):
    if tag is None:
        return [HEAD + b"A1:1 C420jpeg\nFRAME\n", b"YUV4MPEG2 W34 H18 F25:1 \nFRAME\n"]
    return [HEAD + tag + b" A1:1 C420jpeg\nFRAME\n", HEAD + b"A1:1 " + tag + b"\nFRAME\n", HEAD + b"C422 " + tag + b" XYSCSS=422\nFRAME\n"]


@pytest.mark.parametrize("tag,order", TAGS)
def test_y4m_interlace_tag(tag, order):
    for head in _headers(tag):
        data = head + bytes(64)
        if order < 0:
            with pytest.raises(ValueError, match=tag.decode()):
                y4m.interlace(data)
        else:
            assert y4m.interlace(data) == order, head
        # the reference's parser returns for these buffers what it returned before there was vp8host_y4m_interlace
        w, h, rate, first = y4m.parse_header(data)
        assert (w, h, rate, first) == (34, 18, 25, len(head)), head
    lib = api.load_library()
    lib.vp8host_y4m_interlace.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]
    f = C.c_int32(-7)
    assert lib.vp8host_y4m_interlace(b"YUV4MPEG W2 H4 F1:1 It\n", 23, C.byref(f)) == -1       # not the magic word
    assert lib.vp8host_y4m_interlace(b"YUV4MPEG2 W2 H4 F1:1 It", 23, C.byref(f)) == -1        # the header line does not end
    assert lib.vp8host_y4m_interlace(b"YUV4MPEG2 W2 H4 F1:1 Itb\n", 25, C.byref(f)) == -1     # no tag of the format
    assert lib.vp8host_y4m_interlace(None, 0, C.byref(f)) == -1 and f.value == -7
    for cut in range(len(HEAD) + 3):      # a truncated header line: refused, nothing read past the end
        assert lib.vp8host_y4m_interlace((HEAD + b"It\n")[:cut], cut, C.byref(f)) == -1
    # an I inside another tag or behind the header line is no I tag
    assert y4m.interlace(b"YUV4MPEG2 W2 H4 F1:1 XINFO=It\nFRAME\nIb ") == api.FIELDS_PROGRESSIVE


def test_bad_arguments_are_refused():
    f = ref.sequences(16, 16)["moving"][0]
    hist = [p.copy() for p in f]
    for mode, keep in ((-1, 0), (3, 0), (1, 2), (2, -1)):
        with pytest.raises(ValueError):
            api.deinterlace_frame(f, hist, mode, keep, True)
    with pytest.raises(ValueError):
        api.deinterlace_frame(f, None, 2, 0, False)                      # adaptive without history planes
    with pytest.raises(ValueError):
        api.deinterlace_frame([p[:2] for p in f], None, 1, 0, False)     # height 2: the chroma planes have one row
    out, n = api.deinterlace_frame(f, None, 0, 0, False)                 # mode 0: the identity
    assert n == 0 and all(np.array_equal(a, b) for a, b in zip(out, f))


def test_abi_new_entry_points_and_nothing_else_moved():
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.ABI_SYMBOLS, name
    assert C.sizeof(api.DrvConfig) == 88 and api.DrvConfig._fields_[-1][0] == "quality_stats"
    assert C.sizeof(api.DeinterlaceStats) == 12
    lib.vp8hip_abi_version.restype = C.c_int
    assert lib.vp8hip_abi_version() == 4010 == api.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "vp8hip.h")).read() + open(os.path.join(ROOT, "include", "vp8hip_driver.h")).read() + \
        open(os.path.join(ROOT, "include", "vp8hip_host.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+VP8HIP_ABI_VERSION\s+4010\b", hdr)
