"""The tone-mapping rule of include/vp8hip_host.h (vp8host_tonemap_frame, k_tonemap_b) restated in numpy: the per-pixel rule in int64
on four given tables, the tables' formulas in float64, and the frames the tests feed it."""
import numpy as np

P010, I010, BGRA = 4, 5, 18
PQ, HLG = 1, 2
PRIMARIES = np.array([[1701, -602, -75], [-128, 1161, -9], [-19, -103, 1146]], np.int64)      # BT.2020 -> BT.709, times 1024
# include/vp8hip_host.h's colour matrices: offset, then the Y, U and V rows, each R, G, B
COLOUR = [(16, 66, 129, 25, -38, -74, 112, 112, -94, -18), (16, 47, 157, 16, -26, -86, 112, 112, -102, -10),
          (0, 77, 150, 29, -43, -84, 127, 127, -106, -21), (0, 54, 183, 19, -29, -98, 127, 127, -116, -11)]


def tables_ref(transfer, peak):
    """numpy's own evaluation of the tables' formulas -> lin, gain, lo, hi (int64)"""
    e = np.arange(4096) / 4095.0
    P = float(peak)
    if transfer == PQ:
        m1, m2, c1, c2, c3 = 2610 / 16384, 128 * 2523 / 4096, 3424 / 4096, 32 * 2413 / 4096, 32 * 2392 / 4096
        p = e ** (1 / m2)
        D = np.minimum(10000 * (np.maximum(p - c1, 0) / (c2 - c3 * p)) ** (1 / m1), P)
        s = D / P
    else:
        a, b, c = 0.17883277, 0.28466892, 0.55991073
        s = np.where(e <= 0.5, e * e / 3, (np.exp((e - c) / a) + b) / 12)
        D = P * s ** (1.2 + 0.42 * np.log10(P / 1000))
    x, w = D / 203, P / 203
    T = x * (1 + x / (w * w)) / (1 + x)
    lin = np.minimum(2 ** 20 - 1, np.rint(2 ** 20 * s)).astype(np.int64)
    first = int(np.argmax(lin > 0))
    gain = np.rint(65535 * 2.0 ** 20 * T / np.maximum(lin, 1)).astype(np.int64)
    gain[:first] = gain[first]
    j = np.arange(4096)
    lo = np.rint(255 * (j / 65535) ** (1 / 2.4)).astype(np.int64)
    hi = np.rint(255 * (np.minimum(16 * j + 8, 65535) / 65535) ** (1 / 2.4)).astype(np.int64)
    return lin, gain, lo, hi


def grey_o(lin, gain):
    """the grey ramp's linear SDR output: every matrix row sums to 1024, so t = lin"""
    return np.minimum(65535, (np.asarray(lin, np.int64) * np.asarray(gain, np.int64) + 2 ** 19) >> 20)


def c8_of(o, lo, hi):
    o = np.asarray(o, np.int64)
    return np.where(o < 4096, np.asarray(lo, np.int64)[np.minimum(o, 4095)], np.asarray(hi, np.int64)[o >> 4])


def samples_of(fmt, planes, w, h):
    """the ten-bit Y' (h x w), Cb and Cr (h/2 x w/2) a P010 or I010 frame's planes carry, int64"""
    words = [np.ascontiguousarray(p).view(np.uint8).reshape(-1).view("<u2").astype(np.int64) for p in planes]
    if fmt == P010:
        y, c = words[0] >> 6, (words[1] >> 6).reshape(h // 2, w // 2, 2)
        return y.reshape(h, w), c[:, :, 0], c[:, :, 1]
    return (words[0] & 1023).reshape(h, w), (words[1] & 1023).reshape(h // 2, w // 2), (words[2] & 1023).reshape(h // 2, w // 2)


def make_planes(fmt, y, cb, cr, junk=0):
    """the planes of P010 or I010 that carry these ten-bit samples, as flat uint8 arrays; junk (0 .. 63) fills the six bits of every
    word that carry no value"""
    def words(a):
        a = np.asarray(a, np.int64)
        j = np.resize(np.asarray(junk, np.int64), a.shape)      # (an array of junk is repeated or cut to the plane's shape)
        w = (a << 6) | j if fmt == P010 else a | (j << 10)
        return np.ascontiguousarray(w.astype("<u2")).reshape(-1).view(np.uint8)
    if fmt == P010:
        return [words(y), words(np.stack([cb, cr], axis=-1))]
    return [words(y), words(cb), words(cr)]


def c8_picture(y, cb, cr, tables):
    """the per-pixel rule up to c8 -> (h, w, 3) int64, R, G, B"""
    lin, gain, lo, hi = (np.asarray(t, np.int64) for t in tables)
    yy = 38295 * (np.asarray(y, np.int64) - 64) + 4096
    cb2 = np.repeat(np.repeat(np.asarray(cb, np.int64) - 512, 2, axis=0), 2, axis=1)
    cr2 = np.repeat(np.repeat(np.asarray(cr, np.int64) - 512, 2, axis=0), 2, axis=1)
    rgb1 = np.stack([(yy + 55209 * cr2) >> 13, (yy - 6161 * cb2 - 21391 * cr2) >> 13, (yy + 70440 * cb2) >> 13], axis=-1).clip(0, 4095)
    g = gain[rgb1.max(axis=-1)]
    a = lin[rgb1]
    t = np.maximum(0, (a @ PRIMARIES.T + 512) >> 10)
    o = np.minimum(65535, (t * g[..., None] + 2 ** 19) >> 20)
    return c8_of(o, lo, hi)


def bgra_of(c8):
    """the c8 picture as the bytes of a BGRA frame (alpha 255)"""
    h, w, _ = c8.shape
    q = np.full((h, w, 4), 255, np.uint8)
    q[:, :, 0], q[:, :, 1], q[:, :, 2] = c8[:, :, 2], c8[:, :, 1], c8[:, :, 0]
    return q.reshape(-1)


def i420_of(c8, matrix):
    """the BGRA rule of include/vp8hip_host.h on the c8 picture -> (Y, U, V) uint8"""
    m = COLOUR[matrix]
    R, G, B = c8[:, :, 0], c8[:, :, 1], c8[:, :, 2]
    y = m[0] + ((m[1] * R + m[2] * G + m[3] * B + 128) >> 8)
    block = lambda a: a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    u = (block(m[4] * R + m[5] * G + m[6] * B) + 131072 + 512) >> 10
    v = (block(m[7] * R + m[8] * G + m[9] * B) + 131072 + 512) >> 10
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def tonemap_ref(fmt, matrix, w, h, planes, tables):
    return i420_of(c8_picture(*samples_of(fmt, planes, w, h), tables), matrix)


def inputs(w, h, seed=5):
    """the frames a size is tested with, as (name, Y', Cb, Cr): uniform random ten-bit codes (those below 64 and above 940 included), a
    grey ramp, and the eight corners of the Y'CbCr cube tiled over the frame in 2x2 blocks (the saturated BT.2020 primaries drive the
    matrix sums negative: the clamp at 0)"""
    rng = np.random.default_rng(seed + w * 131 + h)
    ch, cw = h // 2, w // 2
    rand = (rng.integers(0, 1024, (h, w)), rng.integers(0, 1024, (ch, cw)), rng.integers(0, 1024, (ch, cw)))
    ramp = (np.linspace(0, 1023, w * h).astype(np.int64).reshape(h, w), np.full((ch, cw), 512), np.full((ch, cw), 512))
    k = np.arange(ch * cw).reshape(ch, cw) % 8
    corners = (np.repeat(np.repeat(np.where(k & 1, 940, 64), 2, axis=0), 2, axis=1), np.where(k & 2, 960, 64), np.where(k & 4, 960, 64))
    return [("random", *rand), ("grey ramp", *ramp), ("cube corners", *corners)]
