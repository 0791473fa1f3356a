"""The canvas rule of include/vp8hip_host.h ("CANVAS") restated in numpy: the background, every present tile in index order through
tests/test_scale_cpu.py's two passes with the library's own tables (vp8host_scale_taps), each plane on its own, into its rectangle,
then copy_with_padding.  tests/test_compose_cpu.py holds vp8host_compose_frame to it byte for byte, tests/test_gpu_compose.py the
kernel.  Also the cases both suites run and the frames they feed them."""
import zlib

import numpy as np

from test_scale_cpu import AREA, LANCZOS, lib_taps, pad_plane, ref_scale_plane_by_tables

BG = (16, 128, 128)


def ref_compose(pw, ph, tiles, frames, bg=BG, taps=lib_taps):
    """tiles[k] = (in_w, in_h, x, y, w, h, filter); frames[k] = (y, u, v) of in_w x in_h (rows may be strided), or None for a tile
    that is absent -> the picture's planes, pw x ph"""
    out = [np.full((ph, pw), bg[0], np.uint8), np.full((ph // 2, pw // 2), bg[1], np.uint8), np.full((ph // 2, pw // 2), bg[2], np.uint8)]
    for (in_w, in_h, x, y, w, h, kind), f in zip(tiles, frames):
        if f is None:
            continue
        assert f[0].shape == (in_h, in_w) and f[1].shape == f[2].shape == (in_h // 2, in_w // 2)
        for p, plane in enumerate(f):
            s = 1 if p else 0
            out[p][y >> s:(y + h) >> s, x >> s:(x + w) >> s] = ref_scale_plane_by_tables(np.ascontiguousarray(plane), w >> s, h >> s, kind, taps)
    return tuple(out)


def ref_surfaces(coded, pw, ph, tiles, frames, bg=BG):
    """... and copy_with_padding of it to the coded size: what the device's current surfaces hold"""
    y, u, v = ref_compose(pw, ph, tiles, frames, bg)
    return pad_plane(y, coded[0], coded[1]), pad_plane(u, coded[0] // 2, coded[1] // 2), pad_plane(v, coded[0] // 2, coded[1] // 2)


def _grid16():
    tiles = [(32, 32, 16 * (k % 4), 16 * (k // 4), 16, 16, AREA) for k in range(15)]
    return tiles + [(62, 62, 6, 10, 2, 2, AREA)]      # one chroma sample, in the middle of an 8-byte unit


_A = (100, 100, 42, 10, 36, 36, LANCZOS)      # touches the picture's right and bottom edges: the padding repeats tile samples
_B = (66, 34, 0, 14, 64, 32, AREA)            # lies over A in x 42 .. 63
# name -> (coded size, picture, tiles, background, indices of absent tiles)
CASES = {
    "identity_area": ((64, 48), (64, 48), [(64, 48, 0, 0, 64, 48, AREA)], BG, ()),
    "identity_lanczos": ((64, 48), (64, 48), [(64, 48, 0, 0, 64, 48, LANCZOS)], BG, ()),
    # the seam at x = 88 falls inside a 64-wide output tile and inside an 8-byte chroma unit
    "grid_area": ((176, 144), (176, 144), [(352, 288, x, y, 88, 72, AREA) for y in (0, 72) for x in (0, 88)], BG, ()),
    "grid_lanczos": ((176, 144), (176, 144), [(352, 288, x, y, 88, 72, LANCZOS) for y in (0, 72) for x in (0, 88)], BG, ()),
    "letterbox_ab": ((80, 48), (78, 46), [_A, _B], (81, 90, 240), ()),
    "letterbox_ba": ((80, 48), (78, 46), [_B, _A], (81, 90, 240), ()),
    "chunking": ((64, 48), (64, 48), [(992, 992, 16, 8, 32, 32, AREA)], BG, ()),      # 31 taps, a source rectangle far larger than LDS
    "sixteen": ((64, 64), (64, 64), _grid16(), BG, (3, 9)),
}


def case_frames(name, seed=0, pitched=False):
    """the case's frames: random planes, tight, or (pitched) luma rows in_w + 12 and chroma rows in_w / 2 + 5 bytes apart, every plane
    in a buffer of exactly its size -- the last row ends with its last sample -- returned as strided views"""
    _, _, tiles, _, absent = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) % 1000 + seed)
    frames = []
    for k, (in_w, in_h, *_rest) in enumerate(tiles):
        if k in absent:
            frames.append(None)
            continue
        planes = []
        for p in range(3):
            w, h = (in_w, in_h) if p == 0 else (in_w // 2, in_h // 2)
            pitch = w + ((12 if p == 0 else 5) if pitched else 0)
            buf = rng.integers(0, 256, pitch * (h - 1) + w, dtype=np.uint8)
            planes.append(np.lib.stride_tricks.as_strided(buf, (h, w), (pitch, 1), writeable=False))
        frames.append(tuple(planes))
    return frames
