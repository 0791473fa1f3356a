"""The overlay rule of include/vp8hip_host.h ("OVERLAYS") restated in numpy, from the header's text: what vp8host_overlay_frame and
k_overlay_prepare / k_overlay_b are held to.  Whole-array arithmetic on int64, true floor division -- no shared code with the C++."""
import numpy as np

# the BGRA paragraph's table: offset, then the Y, U and V rows, each in the order R, G, B
MATRICES = {
    0: (16, (66, 129, 25), (-38, -74, 112), (112, -94, -18)),
    1: (16, (47, 157, 16), (-26, -86, 112), (112, -102, -10)),
    2: (0, (77, 150, 29), (-43, -84, 127), (127, -106, -21)),
    3: (0, (54, 183, 19), (-29, -98, 127), (127, -116, -11)),
}
BGRA, RGBA = 18, 19


def _canvas(layer, x, y, opacity, pw, ph, fmt):
    """the layer laid onto the picture: R, G, B and the effective alpha e per picture pixel (e = 0 where no layer pixel lies)"""
    layer = np.asarray(layer).astype(np.int64)
    lh, lw = layer.shape[:2]
    r_at, b_at = (2, 0) if fmt == BGRA else (0, 2)
    rgb = np.zeros((3, ph, pw), np.int64)
    e = np.zeros((ph, pw), np.int64)
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + lw, pw), min(y + lh, ph)
    if x0 < x1 and y0 < y1:
        part = layer[y0 - y:y1 - y, x0 - x:x1 - x]
        rgb[0, y0:y1, x0:x1] = part[..., r_at]
        rgb[1, y0:y1, x0:x1] = part[..., 1]
        rgb[2, y0:y1, x0:x1] = part[..., b_at]
        e[y0:y1, x0:x1] = (part[..., 3] * opacity + 127) // 255
    return rgb, e


def overlay_frame(layer, x, y, opacity, planes, fmt=BGRA, matrix=0):
    """one layer composed onto (Y, U, V), I420 of the picture size -> new (Y, U, V)"""
    Y, U, V = (np.asarray(p).astype(np.int64) for p in planes)
    ph, pw = Y.shape
    off, cy, cu, cv = MATRICES[matrix]
    rgb, e = _canvas(layer, x, y, opacity, pw, ph, fmt)
    yo = off + ((cy[0] * rgb[0] + cy[1] * rgb[1] + cy[2] * rgb[2] + 128) >> 8)
    out_y = (Y * (255 - e) + yo * e + 127) // 255

    def blocks(a):      # the four pixels of every chroma sample, summed
        return a.reshape(ph // 2, 2, pw // 2, 2).sum(axis=(1, 3))

    E = blocks(e)
    out = [out_y]
    for row, src in ((cu, U), (cv, V)):
        c = row[0] * rgb[0] + row[1] * rgb[1] + row[2] * rgb[2] + 32768
        T = blocks(e * c)
        N = src * 256 * (1020 - E) + T
        assert N.max(initial=0) < 2 ** 31 and N.min(initial=0) >= 0
        out.append(((N + 130560) >> 10) // 255)
    for o in out:
        assert o.min(initial=0) >= 0 and o.max(initial=0) <= 255      # no clamp is needed
    return tuple(o.astype(np.uint8) for o in out)


def overlay_layers(layers, planes):
    """layers = [(pixels, x, y, opacity, fmt, matrix), ...] in slot order, each applied on the result of the one before"""
    for pixels, x, y, opacity, fmt, matrix in layers:
        planes = overlay_frame(pixels, x, y, opacity, planes, fmt, matrix)
    return planes


def pad(planes, W, H):
    """copy_with_padding: sample (x, y) of the coded W x H surface is sample (min(x, pw - 1), min(y, ph - 1)) of the picture"""
    out = []
    for k, p in enumerate(planes):
        w, h = (W, H) if k == 0 else (W // 2, H // 2)
        out.append(np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge"))
    return tuple(out)
