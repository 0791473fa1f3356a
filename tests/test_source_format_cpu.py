"""Source formats, the host side (no GPU): vp8host_convert_frame against the numpy restatement of the rule (tests/source_format_ref.py) and
against round trips that need no restatement, vp8host_source_plane_bytes, and the Y4M header's C tag (vp8host_y4m_colourspace) beside the
reference's parser, which stays what it was."""
import ctypes as C

import numpy as np
import pytest

import source_format_ref as R
from vp8oclenc_amd import api, y4m

SIZES = [(2, 2), (18, 10), (34, 18)]


def convert(fmt, w, h, planes):
    return api.convert_frame(fmt, w, h, planes)


def assert_frames(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape and g.dtype == np.uint8, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


def inputs(fmt, w, h):
    """random, all-zero, all-maximum and, at ten bits, a ramp that ends in 1021, 1022, 1023 (the clamp: 1023 -> 256 -> 255)"""
    top = R.max_sample(fmt)
    shapes = [(h, w), R.chroma_shape(fmt, w, h), R.chroma_shape(fmt, w, h)]
    yield "random", R.random_samples(fmt, w, h, 7 * fmt + w)
    yield "zero", tuple(np.zeros(s, np.int32) for s in shapes)
    yield "maximum", tuple(np.full(s, top, np.int32) for s in shapes)
    if R.depth(fmt) == 10:
        ramp = lambda s: (1023 - (np.arange(s[0] * s[1], dtype=np.int32)[::-1] % 1024)).reshape(s)
        r = tuple(ramp(s) for s in shapes)
        assert {1021, 1022, 1023} <= set(r[0].ravel().tolist()) and all(p.max() == 1023 for p in r)      # (a 2x2 frame's chroma may be one sample)
        yield "ramp", r


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", R.CONVERTED)
def test_convert_frame_equals_the_rule(fmt, w, h):
    for what, (Y, U, V) in inputs(fmt, w, h):
        planes = R.make_planes(fmt, Y, U, V)
        assert [p.size for p in planes] + [0] * (3 - len(planes)) == R.plane_bytes(fmt, w, h)
        assert_frames(convert(fmt, w, h, planes), R.convert_ref(fmt, w, h, planes), f"{R.NAMES[fmt]} {w}x{h} {what}")


def test_the_clamp_is_reached():
    """1023 at ten bits rounds to 256: without the clamp the byte would wrap to 0"""
    for fmt in (R.P010, R.I010, R.I210, R.I410):
        shapes = [(2, 2), R.chroma_shape(fmt, 2, 2), R.chroma_shape(fmt, 2, 2)]
        got = convert(fmt, 2, 2, R.make_planes(fmt, *[np.full(s, 1023) for s in shapes]))
        assert all((p == 255).all() for p in got), R.NAMES[fmt]


@pytest.mark.parametrize("w,h", SIZES)
def test_round_trips_that_need_no_restatement(w, h):
    rng = np.random.default_rng(w * 100 + h)
    frame = (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
             rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))
    y, u, v = frame
    # NV12: the frame's chroma interleaved
    nv12 = [y.ravel(), np.stack([u, v], axis=-1).ravel()]
    assert_frames(convert(R.NV12, w, h, nv12), frame, "NV12")
    # P010 = v << 8 (the value in the top ten bits), I010 = v << 2
    p010 = [(y.astype(np.uint16) << 8).astype("<u2").ravel().view(np.uint8),
            (np.stack([u, v], axis=-1).astype(np.uint16) << 8).astype("<u2").ravel().view(np.uint8)]
    assert_frames(convert(R.P010, w, h, p010), frame, "P010")
    i010 = [(p.astype(np.uint16) << 2).astype("<u2").ravel().view(np.uint8) for p in frame]
    assert_frames(convert(R.I010, w, h, i010), frame, "I010")
    # 4:2:2 and 4:4:4 with the frame's chroma replicated
    i422 = [y.ravel(), np.repeat(u, 2, axis=0).ravel(), np.repeat(v, 2, axis=0).ravel()]
    assert_frames(convert(R.I422, w, h, i422), frame, "I422")
    i444 = [y.ravel()] + [np.repeat(np.repeat(c, 2, axis=0), 2, axis=1).ravel() for c in (u, v)]
    assert_frames(convert(R.I444, w, h, i444), frame, "I444")
    # the makers of source_format_ref.py build the same planes
    for fmt, planes in ((R.NV12, nv12), (R.P010, p010), (R.I010, i010), (R.I422, i422), (R.I444, i444)):
        for a, b in zip(R.from_i420(fmt, *frame), planes):
            assert np.array_equal(a, b), R.NAMES[fmt]
    for fmt in (R.I210, R.I410):
        assert_frames(convert(fmt, w, h, R.from_i420(fmt, *frame)), frame, R.NAMES[fmt])


@pytest.mark.parametrize("w,h", SIZES)
def test_bits_that_carry_no_value_are_ignored(w, h):
    rng = np.random.default_rng(5)
    junk = rng.integers(1, 64, (h, w))
    for fmt in (R.P010, R.I010, R.I210, R.I410):      # P010: the low six bits; the others: the high six
        s = R.random_samples(fmt, w, h, 3)
        clean, dirty = R.make_planes(fmt, *s), R.make_planes(fmt, *s, junk=junk)
        assert any(not np.array_equal(a, b) for a, b in zip(clean, dirty))
        assert_frames(convert(fmt, w, h, dirty), convert(fmt, w, h, clean), R.NAMES[fmt])


def test_source_plane_bytes():
    lib = api.load_library()
    lib.vp8host_source_plane_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    b = (C.c_size_t * 3)()
    for w, h in SIZES + [(1920, 1080), (16384, 16384)]:
        for fmt in R.ALL:
            assert lib.vp8host_source_plane_bytes(fmt, w, h, b) == 0
            assert list(b) == R.plane_bytes(fmt, w, h), (R.NAMES[fmt], w, h)
            assert api.source_plane_bytes(fmt, w, h) == list(b)
    assert list(api.source_plane_bytes(R.NV12, 1920, 1080)) == [1920 * 1080, 1920 * 540, 0]
    assert list(api.source_plane_bytes(R.I410, 34, 18)) == [34 * 18 * 2] * 3
    for fmt, w, h in ((8, 16, 16), (-1, 16, 16), (R.NV12, 17, 16), (R.NV12, 16, 15), (R.I420, 0, 16), (R.I444, 16, -2)):
        assert lib.vp8host_source_plane_bytes(fmt, w, h, b) == -1, (fmt, w, h)
    assert lib.vp8host_source_plane_bytes(R.NV12, 16, 16, None) == -1
    lib.vp8host_convert_frame.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert lib.vp8host_convert_frame(8, 16, 16, p, p, p, p, p, p) == -1
    assert lib.vp8host_convert_frame(R.I444, 15, 16, p, p, p, p, p, p) == -1
    assert lib.vp8host_convert_frame(R.I444, 16, 16, p, p, None, p, p, p) == -1
    assert lib.vp8host_convert_frame(R.NV12, 16, 16, p, p, None, p, p + 1024, p + 2048) == 0      # two planes: the third is not read


TAGS = [(None, R.I420), ("C420", R.I420), ("C420jpeg", R.I420), ("C420mpeg2", R.I420), ("C420paldv", R.I420), ("C422", R.I422), ("C444", R.I444),
        ("C420p10", R.I010), ("C422p10", R.I210), ("C444p10", R.I410), ("Cmono", -1), ("C420p12", -1), ("C444alpha", -1), ("C444p16", -1),
        ("C42", -1), ("C4200", -1)]


def headers(tag):
    """the tag after W / H / F (where ffmpeg writes it) and in front of them"""
    if tag is None:
        return [b"YUV4MPEG2 W34 H18 F25:1 Ip A1:1\nFRAME\n"]
    t = tag.encode()
    return [b"YUV4MPEG2 W34 H18 F25:1 Ip A1:1 " + t + b" XYSCSS=420\nFRAME\n", b"YUV4MPEG2 " + t + b" W34 H18 F25:1 Ip\nFRAME\n",
            b"YUV4MPEG2 W34 H18 F25:1 " + t + b"\nFRAME\n"]


@pytest.mark.parametrize("tag,fmt", TAGS)
def test_y4m_colourspace(tag, fmt):
    for head in headers(tag):
        data = head + bytes(64)
        if fmt < 0:
            with pytest.raises(ValueError, match=tag):
                y4m.colourspace(data)
        else:
            assert y4m.colourspace(data) == fmt, head
    lib = api.load_library()
    lib.vp8host_y4m_colourspace.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]
    f = C.c_int32(-7)
    assert lib.vp8host_y4m_colourspace(b"YUV4MPEG W2 H2 F1:1 C444\n", 25, C.byref(f)) == -1      # not the magic word
    assert lib.vp8host_y4m_colourspace(b"YUV4MPEG2 W2 H2 F1:1 C444", 25, C.byref(f)) == -1       # the header line does not end
    assert lib.vp8host_y4m_colourspace(None, 0, C.byref(f)) == -1 and f.value == -7
    # a C inside another tag or behind the header line is no C tag
    assert y4m.colourspace(b"YUV4MPEG2 W2 H2 F1:1 XCOLORRANGE=C444\nFRAME\nC422 ") == R.I420


# what vp8host_y4m_parse_header returned for these buffers before vp8host_y4m_colourspace existed: (width, height, rate, offset)
@pytest.mark.parametrize("tag,fmt", TAGS)
def test_the_reference_parser_is_what_it_was(tag, fmt):
    for head in headers(tag):
        w, h, rate, first = y4m.parse_header(head + bytes(64))
        assert (w, h, rate) == (34, 18, 25), head
        assert first == len(head), head
