"""The temporal filter of the hidden alternate reference frame restated in numpy from the TEXT of include/vp8hip_host.h (not from
vp8host_arf_filter_frame's C++): the extension, the search with its 29-bit key, the block weight, the per-sample modifier and the
rounded division.  tests/test_arf_cpu.py holds the host function to it, tests/test_gpu_arf.py the kernel.  Also here: the picture
sequences those tests feed, the hidden-frame schedule of the tools, and the CPU oracle's backend for the frame loop with hidden frames."""
import numpy as np

MAX_FRAMES = 7
THRESH_LOW, THRESH_HIGH = 10000, 20000


def _extended(plane, we, he):
    h, w = plane.shape
    return np.pad(plane, ((0, he - h), (0, we - w)), mode="edge").astype(np.int64)


def search(centre_tile, other_ext, x0, y0):
    """the winner of the full-pel search of one 16x16 tile in one extended luma plane -> (dx, dy, sse)"""
    he, we = other_ext.shape
    best = None
    for dy in range(-8, 8):
        if y0 + dy < 0 or y0 + dy + 16 > he:
            continue
        for dx in range(-8, 8):
            if x0 + dx < 0 or x0 + dx + 16 > we:
                continue
            blk = other_ext[y0 + dy:y0 + dy + 16, x0 + dx:x0 + dx + 16]
            sad = int(np.abs(centre_tile - blk).sum())
            key = (sad, abs(dx) + abs(dy), dy, dx)
            if best is None or key < best:
                best = key
    _, _, dy, dx = best
    blk = other_ext[y0 + dy:y0 + dy + 16, x0 + dx:x0 + dx + 16]
    return dx, dy, int(((centre_tile - blk) ** 2).sum())


def block_weight(sse):
    return 2 if sse < THRESH_LOW else (1 if sse < THRESH_HIGH else 0)


def _accumulate(o, p, bw, strength, acc, count):
    r = (1 << (strength - 1)) if strength else 0
    d = o - p
    m = (3 * d * d + r) >> strength
    m = 16 - np.minimum(m, 16)
    count += m * bw
    acc += m * bw * p


def filter_frame(frames, centre, strength):
    """frames: list of (Y, U, V) uint8 planes of one even size -> ((Y, U, V) filtered, weights[3], vectors[tiles][n][2])"""
    n = len(frames)
    assert 1 <= n <= MAX_FRAMES and 0 <= centre < n and 0 <= strength <= 6
    h, w = frames[0][0].shape
    assert w % 2 == 0 and h % 2 == 0
    tw, th = (w + 15) // 16, (h + 15) // 16
    we, he = tw * 16, th * 16
    ext = [(_extended(y, we, he), _extended(u, we // 2, he // 2), _extended(v, we // 2, he // 2)) for y, u, v in frames]
    out = [np.zeros((he, we), np.uint8), np.zeros((he // 2, we // 2), np.uint8), np.zeros((he // 2, we // 2), np.uint8)]
    weights = [0, 0, 0]
    vectors = np.zeros((tw * th, n, 2), np.int8)
    for ty in range(th):
        for tx in range(tw):
            x0, y0 = tx * 16, ty * 16
            cx0, cy0 = x0 // 2, y0 // 2
            o = [ext[centre][0][y0:y0 + 16, x0:x0 + 16], ext[centre][1][cy0:cy0 + 8, cx0:cx0 + 8], ext[centre][2][cy0:cy0 + 8, cx0:cx0 + 8]]
            acc = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
            cnt = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
            for k in range(n):
                if k == centre:
                    dx, dy, bw = 0, 0, 2
                else:
                    dx, dy, sse = search(o[0], ext[k][0], x0, y0)
                    bw = block_weight(sse)
                    weights[bw] += 1
                vectors[ty * tw + tx, k] = (dx, dy)
                if not bw:
                    continue
                _accumulate(o[0], ext[k][0][y0 + dy:y0 + dy + 16, x0 + dx:x0 + dx + 16], bw, strength, acc[0], cnt[0])
                ux, uy = cx0 + (dx >> 1), cy0 + (dy >> 1)
                for p in (1, 2):
                    _accumulate(o[p], ext[k][p][uy:uy + 8, ux:ux + 8], bw, strength, acc[p], cnt[p])
            assert all((c >= 32).all() and (c <= 224).all() for c in cnt) and all((a < 65536).all() for a in acc)
            out[0][y0:y0 + 16, x0:x0 + 16] = (acc[0] + cnt[0] // 2) // cnt[0]
            out[1][cy0:cy0 + 8, cx0:cx0 + 8] = (acc[1] + cnt[1] // 2) // cnt[1]
            out[2][cy0:cy0 + 8, cx0:cx0 + 8] = (acc[2] + cnt[2] // 2) // cnt[2]
    planes = (np.ascontiguousarray(out[0][:h, :w]), np.ascontiguousarray(out[1][:h // 2, :w // 2]), np.ascontiguousarray(out[2][:h // 2, :w // 2]))
    return planes, weights, vectors


# ---- pictures ---------------------------------------------------------------------------------------------------------------------------
def texture(w, h, seed, margin=40):
    """a smooth but busy picture larger than the frame by `margin` on every side: windows of it translate without wrapping"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h + 2 * margin, 0:w + 2 * margin]
    y = 128 + 50 * np.sin(xx / 3.7 + seed) * np.cos(yy / 4.3) + 40 * np.sin((xx + 2 * yy) / 9.1) + rng.integers(-12, 13, xx.shape)
    u = 128 + 40 * np.sin(xx / 11.0) + 20 * np.cos(yy / 7.0 + seed)
    v = 128 + 40 * np.cos(xx / 8.0 + 1) - 20 * np.sin(yy / 13.0)
    return [np.clip(p, 0, 255).astype(np.uint8) for p in (y, u, v)]


def window_of(tex, w, h, ox, oy, margin=40):
    """the w x h frame whose top-left luma sample is (margin + ox, margin + oy) of the texture; ox, oy even (4:2:0 stays exact);
    chroma is the texture's chroma subsampled by dropping"""
    assert ox % 2 == 0 and oy % 2 == 0
    y, u, v = tex
    a, b = margin + ox, margin + oy
    return (np.ascontiguousarray(y[b:b + h, a:a + w]), np.ascontiguousarray(u[b:b + h:2, a:a + w:2]), np.ascontiguousarray(v[b:b + h:2, a:a + w:2]))


def translating(w, h, n, step, seed=1):
    """n frames of one texture; frame k is displaced by k * step = (sx, sy) luma samples (even numbers)"""
    tex = texture(w, h, seed)
    return [window_of(tex, w, h, k * step[0], k * step[1]) for k in range(n)]


def noisy_still(w, h, n, amplitude, seed=2):
    """one clean picture under independent uniform noise of +-amplitude per frame -> (frames, clean)"""
    rng = np.random.default_rng(seed)
    clean = window_of(texture(w, h, seed), w, h, 0, 0)
    frames = [tuple(np.clip(p.astype(np.int64) + rng.integers(-amplitude, amplitude + 1, p.shape), 0, 255).astype(np.uint8) for p in clean)
              for _ in range(n)]
    return frames, clean


def wild(w, h, n, seed=3):
    """frames that share a drifting picture, with noise, a cut before the last frame and a flat patch: every branch of the rule"""
    rng = np.random.default_rng(seed)
    tex, other = texture(w, h, seed), texture(w, h, seed + 100)
    out = []
    for k in range(n):
        f = window_of(other if (n > 2 and k == n - 1) else tex, w, h, 2 * (k % 4), 2 * ((k * 3) % 5) - 4)
        f = [np.clip(p.astype(np.int64) + rng.integers(-6, 7, p.shape), 0, 255).astype(np.uint8) for p in f]
        f[0][: h // 3, : w // 3] = 90      # flat: every candidate there ties
        out.append(tuple(np.ascontiguousarray(p) for p in f))
    return out


# ---- where the tools put hidden frames -----------------------------------------------------------------------------------------------------
def schedule(total, gop_size, period, max_frames=7):
    """The tools' placement (scripts/native/y4m_to_ivf -arf PERIOD[:FRAMES[:STRENGTH]]): inside every GOP [g, g + gop_size) the frames form groups of
    `period`; a hidden frame is coded in front of each group's first frame -- for the GOP's first group behind the key frame, since in
    front of it there is no reference of this GOP -- centred on the group's last frame, its window of max_frames frames clipped to the
    GOP and to the file.  -> {shown frame index t: (window start, frames in the window, centre's index in the window, where)} with where =
    'before' (the hidden frame precedes frame t) or 'after' (it follows the key frame t)."""
    out = {}
    for g in range(0, total, gop_size):
        end = min(g + gop_size, total)
        for first in range(g, end, period):
            last = min(first + period, end) - 1
            if last == g:      # a group that is the key frame alone
                continue
            half = max_frames // 2
            lo, hi = max(g, last - half), min(end - 1, last + half)
            out[first] = (lo, hi - lo + 1, last - lo, "after" if first == g else "before")
    return out


# ---- the CPU oracle as the frame loop's backend -------------------------------------------------------------------------------------------
def oracle_backend(w, h, ssim_target=-1.0):
    """tests/oracle_lib.Oracle with the two calls of a hidden frame: arf_filter (the restatement above) and loop_filter_hidden (the
    reconstruction becomes ALTREF and LAST stays; the oracle's own rotation does the copy)"""
    from oracle_lib import Oracle

    class ArfOracle(Oracle):
        def arf_filter(self, frames, centre, strength):
            planes, self.arf_weights, _ = filter_frame(frames, centre, strength)
            self.upload_current(*planes)
            return planes

        def loop_filter(self):
            super().loop_filter()
            self._last = tuple(p.copy() for p in self.download_last())

        def upload_last(self, y, u, v):
            super().upload_last(y, u, v)
            self._last = (np.ascontiguousarray(y).copy(), np.ascontiguousarray(u).copy(), np.ascontiguousarray(v).copy())

        def loop_filter_hidden(self):
            keep = self._last
            Oracle.loop_filter(self)                   # the filtered reconstruction is the oracle's LAST for a moment ...
            self.hidden_recon = tuple(p.copy() for p in self.download_last())
            # ... a transform with prev_is_altref = 1 copies LAST (and its pyramid) into ALTREF; what it codes is thrown away
            self.inter_transform(0, 1, 0, 0)
            super().upload_last(*keep)                 # ... and LAST is what it was
            self._lf = dict(self._lf, recon_Y=keep[0], recon_U=keep[1], recon_V=keep[2])

    return ArfOracle(w, h, ssim_target)


# ---- a sequence with hidden frames through the frame loop ------------------------------------------------------------------------------
def noisy_pan(w, h, n, seed, amplitude=5):
    """a texture that drifts two samples per frame under fresh noise: what a hidden frame is for"""
    rng = np.random.default_rng(seed)
    tex = texture(w, h, seed, margin=8 + 2 * n)
    out = []
    for k in range(n):
        f = window_of(tex, w, h, 2 * k, 0, margin=8)
        out.append(tuple(np.ascontiguousarray(np.clip(p.astype(np.int64) + rng.integers(-amplitude, amplitude + 1, p.shape), 0, 255).astype(np.uint8))
                         for p in f))
    return out


def events(total, placement):
    """the order of calls for `placement` = {t: (lo, n, centre, 'before' | 'after')}: ('hidden', t, lo, n, centre) and ('shown', t)"""
    out = []
    for t in range(total):
        spec = placement.get(t)
        if spec and spec[3] == "before":
            out.append(("hidden", t) + tuple(spec[:3]))
        out.append(("shown", t))
        if spec and spec[3] == "after":
            out.append(("hidden", t) + tuple(spec[:3]))
    return out


def oracle_loop(frames, placement, strength, conformant=False, **cfg):
    """The CPU oracle through vp8oclenc_amd.driver.InterPathDriver with hidden frames where `placement` says -> a list of records
    dict(kind, t, key, out, recon) in stream order: out = the frame's outputs as tests/bitstream_cases.expected_frame takes them,
    recon = the loop-filtered reconstruction (of a hidden frame: what became ALTREF)."""
    from oracle_lib import Oracle
    from vp8oclenc_amd.driver import InterPathDriver
    h, w = frames[0][0].shape
    Oracle.lib().vp8o_set_conformant_stream(1 if conformant else 0)
    try:
        be = oracle_backend(w, h, cfg.get("ssim_target", -1.0))
        drv = InterPathDriver(be, w, h, **cfg)
        rec = []
        for ev in events(len(frames), placement):
            if ev[0] == "shown":
                out = drv.encode_frame(*frames[ev[1]])
                key = out is None
                rec.append(dict(kind="shown", t=ev[1], key=key, out=drv.last_key if key else out, recon=tuple(p.copy() for p in be.download_last())))
            else:
                _, t, lo, n, centre = ev
                out = drv.encode_hidden(frames[lo:lo + n], centre, strength)
                rec.append(dict(kind="hidden", t=t, key=False, out=out, recon=be.hidden_recon, window=(lo, n, centre), weights=list(be.arf_weights)))
        be.close()
        return rec
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)


def record_bytes(rec, w, h, partitions):
    """the bytes of a record's frame: coefficient partitions by the entropy oracle, first partition by the host coder for a hidden frame
    (the reference knows none) and by the reference's own where it is built for the others.  So for a HIDDEN frame the expected first
    partition is the project's own host coder (vp8_bitstream.cpp): a byte comparison against it checks the device coder against the host
    coder, and with host_bitstream = 1 the code against itself.  What is independent of both coders is the decoding: tests/vp8_parse.py
    on the header bits (tests/test_arf_cpu.py) and tests/vp8_decode.py on whole conformant streams, reconstruction by reconstruction."""
    from bitstream_cases import expected_frame
    return expected_frame(w, h, rec["out"], rec["key"], partitions, use_reference=rec["kind"] != "hidden")
