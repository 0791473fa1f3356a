"""The denoiser's rule (include/vp8hip_host.h, vp8hip_set_denoise) restated in numpy, independently of the C++ and of the kernel, and the
input sequences that make every branch of it occur.  Shared by tests/test_denoise_cpu.py and tests/test_gpu_denoise.py."""
import numpy as np

SUM_Y, SAD_Y, SUM_C = 512, 2560, 128


def _steps(S, R, k):
    d = R.astype(np.int32) - S.astype(np.int32)
    a = np.abs(d)
    m = np.where(a <= 2 + k, a, np.where(a <= 7, 2 + k, np.where(a <= 15, 3 + k, 5 + k)))
    return np.sign(d) * m, a


def _blocks(x, n):
    h, w = x.shape
    return x.reshape(h // n, n, w // n, n).sum(axis=(1, 3))


def denoise(src, hist, level):
    """one frame with a history -> (out (Y, U, V), info); info: T, sad, filtered [mbh, mbw], filtered_u, filtered_v"""
    cy, ay = _steps(src[0], hist[0], level)
    T, sad = _blocks(cy, 16), _blocks(ay, 16)
    f = (np.abs(T) <= SUM_Y) & (sad <= SAD_Y)
    out = [np.where(np.kron(f, np.ones((16, 16), bool)), src[0] + cy, src[0]).astype(np.uint8)]
    info = {"T": T, "sad": sad, "filtered": f}
    for p, name in ((1, "u"), (2, "v")):
        c, _ = _steps(src[p], hist[p], level)
        fc = f & (np.abs(_blocks(c, 8)) <= SUM_C)
        out.append(np.where(np.kron(fc, np.ones((8, 8), bool)), src[p] + c, src[p]).astype(np.uint8))
        info["filtered_" + name] = fc
    return out, info


class Denoiser:
    """a context's denoiser: level, history, restart; take(frame) -> (out, macroblocks filtered, info or None for a frame that passed through)"""

    def __init__(self, level):
        self.level = level
        self.hist = None

    def restart(self):
        self.hist = None

    def take(self, frame):
        frame = [np.asarray(p, np.uint8) for p in frame]
        if not self.level:
            return [p.copy() for p in frame], 0, None
        if self.hist is None:
            out, n, info = [p.copy() for p in frame], 0, None
        else:
            out, info = denoise(frame, self.hist, self.level)
            n = int(info["filtered"].sum())
        self.hist = [p.copy() for p in out]
        return out, n, info


def _picture(rng, w, h, lo=40, hi=200):
    """a smooth picture with some structure, well inside (lo, hi) so that noise and steps never clip"""
    yy, xx = np.mgrid[0:h, 0:w]
    base = (lo + hi) / 2 + (hi - lo) / 4 * (np.sin(xx / 7.0) + np.cos(yy / 5.0)) / 2 + rng.integers(-6, 7, (h, w))
    return np.clip(base, lo, hi).astype(np.int32)


def sequences(w, h, seed=1, frames=5):
    """name -> list of `frames` frames (Y, U, V) uint8 of the coded size w x h; what each is for: tests/test_denoise_cpu.py"""
    rng = np.random.default_rng(seed)
    cw, ch = w // 2, h // 2
    Y, U, V = _picture(rng, w, h), _picture(rng, cw, ch, 90, 160), _picture(rng, cw, ch, 90, 160)
    u8 = lambda *p: [np.ascontiguousarray(x, np.uint8) for x in p]
    noise = lambda shape, amp: rng.integers(-amp, amp + 1, shape)
    seq = {}
    # a static picture, then the picture plus noise of amplitude <= 3: every |d| <= 3 <= 2 + k, the output is the history
    seq["static_noise"] = [u8(Y, U, V)] + [u8(Y + noise(Y.shape, 3), U + noise(U.shape, 3), V + noise(V.shape, 3)) for _ in range(frames - 1)]
    # an 8 wide bright stripe that moves 8 samples per frame: in a macroblock it moves inside of, as many samples fall as rise (T = 0) and
    # the SAD bound alone says "copied"
    s = []
    for t in range(frames):
        y = np.full((h, w), 60, np.int32)
        x0 = (8 * t) % w
        y[:, x0:x0 + 8] = 220
        s.append(u8(y, np.full((ch, cw), 128), np.full((ch, cw), 128)))
    seq["moving_stripe"] = s
    # the whole picture 5 brighter every frame: sad = 1280 passes, |T| >= 256 * 3 does not
    seq["brightness_step"] = [u8(Y + 5 * t, U, V) for t in range(frames)]
    # luma and V stand still, U is 3 higher every frame: |T_u| = 64 * 3 > 128 copies the U block of a filtered macroblock
    seq["chroma_step"] = [u8(Y, U + 3 * t, V) for t in range(frames)]
    # left: noise on a static picture; right of the first macroblock column: brightness steps -- some filtered, some not
    s = []
    for t in range(frames):
        y = Y + (noise(Y.shape, 2) if t else 0)
        y[:, 16:] = Y[:, 16:] + 5 * t
        s.append(u8(y, U + (noise(U.shape, 2) if t else 0), V))
    seq["mixed"] = s
    # anything goes: noise of amplitude 12 on a slowly drifting picture, every branch of the step in one frame
    seq["wild"] = [u8(np.clip(Y + t + noise(Y.shape, 12), 0, 255), np.clip(U + noise(U.shape, 5), 0, 255), np.clip(V - t + noise(V.shape, 9), 0, 255))
                   for t in range(frames)]
    return seq
