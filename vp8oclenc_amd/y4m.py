"""YUV4MPEG2, the reference's input format (OpenYUV420FileAndParseHeader, init.h:1610-1737; get_yuv420_frame,
encIO.h:203-254), read the way the reference reads it: the header by the native restatement (vp8host_y4m_parse_header),
frames as tight I420 of the header's size, each followed by the next frame's 6-byte FRAME line whose bytes 0 and 4 the
reference checks.  What the reference never looks at, the header's C tag, is read beside it (vp8host_y4m_colourspace): a file of
4:2:2, 4:4:4 or 10-bit frames is read as what it is (Y4mFile.format, Y4mFile.planes) and converted on the device
(vp8hip_set_source_format)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import api


def parse_header(data: bytes):
    """(width, height, framerate, offset of the first frame's samples); raises on what the reference refuses"""
    lib = api.load_library()
    lib.vp8host_y4m_parse_header.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]
    w, h, f, off = C.c_int32(), C.c_int32(), C.c_int32(), C.c_size_t()
    if lib.vp8host_y4m_parse_header(data, len(data), C.byref(w), C.byref(h), C.byref(f), C.byref(off)) != 0:
        raise ValueError("not a YUV4MPEG2 stream the reference accepts (magic word, W / H / F tags ended by spaces, a plain FRAME line)")
    return w.value, h.value, f.value, off.value


def colourspace(data: bytes) -> int:
    """the source format (api.FORMAT_*) the header's C tag names: I420 without one; raises ValueError, naming the tag, for a
    colourspace the encoder cannot take (Cmono, C444alpha, 12 and 16 bits, ...)"""
    lib = api.load_library()
    lib.vp8host_y4m_colourspace.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]
    fmt = C.c_int32()
    if lib.vp8host_y4m_colourspace(data, len(data), C.byref(fmt)) != 0:
        line = bytes(data).split(b"\n", 1)[0].split(b" ")
        tag = next((t.decode("latin-1") for t in line[1:] if t.startswith(b"C")), None)
        raise ValueError(f"colourspace tag {tag}: not one of C420*, C422, C444, C420p10, C422p10, C444p10" if tag
                         else "not a YUV4MPEG2 header line")
    return fmt.value


def interlace(data: bytes) -> int:
    """the field order (api.FIELDS_*) the header's I tag names: progressive without one, for Ip and for I?; raises ValueError, naming
    the tag, for Im (mixed) and anything else"""
    lib = api.load_library()
    lib.vp8host_y4m_interlace.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]
    order = C.c_int32()
    if lib.vp8host_y4m_interlace(data, len(data), C.byref(order)) != 0:
        line = bytes(data).split(b"\n", 1)[0].split(b" ")
        tag = next((t.decode("latin-1") for t in line[1:] if t.startswith(b"I")), None)
        raise ValueError(f"interlace tag {tag}: not one of Ip, I?, It, Ib" if tag else "not a YUV4MPEG2 header line")
    return order.value


class Y4mFile:
    """frames of a .y4m file: .W, .H (the SOURCE size: hand them to an encoder created for the padded size with
    src_width / src_height), .framerate, .n, .format (api.FORMAT_*, from the C tag, or `fmt` for a file whose frames are NV12 /
    P010, which the header cannot say), .frame(t) -> (y, u, v) of an I420 file, .planes(t) -> the format's planes as flat uint8"""

    def __init__(self, path: str, fmt=None):
        self.m = np.memmap(path, np.uint8, "r")
        self.W, self.H, self.framerate, self.first = parse_header(bytes(self.m[:4096]))
        if self.W % 2 or self.H % 2:
            raise ValueError("odd frame sizes are not I420 the reference can read")
        self.format = colourspace(bytes(self.m[:4096])) if fmt is None else api.source_format(fmt)
        self.plane_bytes = api.source_plane_bytes(self.format, self.W, self.H)
        self.fsz = sum(self.plane_bytes)
        self.n = (len(self.m) - self.first + 6) // (self.fsz + 6)
        lib = api.load_library()
        lib.vp8host_y4m_frame_marker_ok.argtypes = [C.c_char_p]
        self._ok = lib.vp8host_y4m_frame_marker_ok

    def _bytes(self, t: int):
        if not 0 <= t < self.n:
            raise IndexError(f"frame {t} of {self.n}")
        a = self.first + t * (self.fsz + 6)
        if t > 0 and not self._ok(bytes(self.m[a - 6:a])):
            raise ValueError(f"broken stream before frame {t}")          # encIO.h:245-248
        return self.m[a:a + self.fsz]

    def planes(self, t: int):
        """frame t as the file's format has it: two or three flat uint8 arrays (16-bit samples as their little-endian bytes)"""
        b = self._bytes(t)
        n0, n1, n2 = self.plane_bytes
        return [np.ascontiguousarray(p) for p in (b[:n0], b[n0:n0 + n1], b[n0 + n1:])[:3 if n2 else 2]]

    def frame(self, t: int):
        if self.format != api.FORMAT_I420:
            raise ValueError(f"a {api.source_format_name(self.format)} file has no I420 frames: planes(t), and vp8drv_set_source_format")
        b = self._bytes(t)
        W, H = self.W, self.H
        return (np.ascontiguousarray(b[:W * H].reshape(H, W)), np.ascontiguousarray(b[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)),
                np.ascontiguousarray(b[W * H * 5 // 4:].reshape(H // 2, W // 2)))


def write_y4m(path: str, frames, framerate: int = 30, tag: str = "C420jpeg XYSCSS=420JPEG", size=None):
    """a .y4m as ffmpeg writes it (for tests and tools).  tag: the colourspace tag, for frames that are another format's planes
    (then `size` = (W, H), which flat planes do not say)"""
    frames = list(frames)
    H, W = (size[1], size[0]) if size else frames[0][0].shape
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{W} H{H} F{framerate}:1 Ip A1:1 {tag}\n".encode())
        for planes in frames:
            f.write(b"FRAME\n")
            for p in planes:
                f.write(np.ascontiguousarray(p).tobytes())
