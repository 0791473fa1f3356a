"""The tools' crop and rotation options: scripts/native/y4m_to_ivf -crop W:H:X:Y -rotate N [-mirror] on a Y4M file of surfaces writes
the IVF file the program writes for the Y4M file of the cropped, rotated frames, scripts/encode_ivf.py --surface --crop --rotate does
the same on a raw file, and a window that does not fit is refused before anything is coded."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import geometry_ref as ref
from test_gpu_deinterlace_tools import write_y4m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE, RAW, ORIGIN, FRAMES = (64, 80), (48, 64), (2, 6), 5      # the window of 48x64 at (2, 6) turned once: a picture of 64x48


def videos():
    """surfaces whose window drifts (the inter frames find motion), and the frames a transcoder would have cropped and turned by hand"""
    rng = np.random.default_rng(91)
    big = ref.raw_frame(RAW[0] + 2 * FRAMES, RAW[1] + 2 * FRAMES, seed=92)
    surfaces, frames = [], {}
    for t in range(FRAMES):
        f = [big[0][2 * t:2 * t + RAW[1], 2 * t:2 * t + RAW[0]], big[1][t:t + RAW[1] // 2, t:t + RAW[0] // 2], big[2][t:t + RAW[1] // 2, t:t + RAW[0] // 2]]
        s = ref.surface(ref.I420, SURFACE[0], SURFACE[1], ref.tight_pitch(ref.I420, SURFACE[0]), rng)
        for p, (hs, vs, _) in enumerate(ref.TABLE[ref.I420]):
            s[p][ORIGIN[1] >> vs:(ORIGIN[1] >> vs) + f[p].shape[0], ORIGIN[0] >> hs:(ORIGIN[0] >> hs) + f[p].shape[1]] = f[p]
        surfaces.append(s)
        for key in ((1, 0), (3, 1), (0, 0)):
            frames.setdefault(key, []).append(ref.orient(f, *key))
    return surfaces, frames


def test_y4m_to_ivf_crop_and_rotate(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "y4m_to_ivf")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", "y4m_to_ivf.cpp"), "-o", exe,
                    "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    surfaces, frames = videos()
    write_y4m(str(tmp_path / "surfaces.y4m"), surfaces, "")
    for key, v in frames.items():
        write_y4m(str(tmp_path / f"by_hand_{key[0]}{key[1]}.y4m"), v, "")

    def run(src, out, *opts, ok=True):
        r = subprocess.run([exe, str(tmp_path / src), str(tmp_path / out), "-g", "3", "-partitions", "2"] + list(opts), capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read() if ok else r.stderr

    crop = f"{RAW[0]}:{RAW[1]}:{ORIGIN[0]}:{ORIGIN[1]}"
    want = run("by_hand_10.y4m", "want.ivf")
    assert len(want) > 32 + 12 * FRAMES and int.from_bytes(want[12:14], "little") == 64 and int.from_bytes(want[14:16], "little") == 48
    assert run("surfaces.y4m", "got.ivf", "-crop", crop, "-rotate", "90") == want
    assert run("surfaces.y4m", "got31.ivf", "-crop", crop, "-rotate", "270", "-mirror") == run("by_hand_31.y4m", "want31.ivf")
    assert run("surfaces.y4m", "got00.ivf", "-crop", crop) == run("by_hand_00.y4m", "want00.ivf")
    assert want != run("by_hand_31.y4m", "want31.ivf")
    # with -resize: the picture behind the turn is what is scaled
    assert run("surfaces.y4m", "small.ivf", "-crop", crop, "-rotate", "90", "-resize", "32x24") == run("by_hand_10.y4m", "small_want.ivf", "-resize", "32x24")
    for bad in ("48:64:3:6", "48:64:2:18", "48:64:18:6", "0:64:2:6"):      # odd, below the surface, beyond its right edge, empty
        assert "-crop" in run("surfaces.y4m", "no.ivf", "-crop", bad, ok=False)
    assert "-rotate" in run("surfaces.y4m", "no.ivf", "-rotate", "45", ok=False)


def test_encode_ivf_surface_crop_and_rotate(tmp_path):
    surfaces, frames = videos()
    for name, v in (("surfaces.yuv", surfaces), ("by_hand.yuv", frames[(1, 0)])):
        with open(tmp_path / name, "wb") as f:
            for planes in v:
                for p in planes:
                    f.write(np.ascontiguousarray(p).tobytes())

    def run(out, *opts):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / out), "--frames", str(FRAMES), "--gop", "3", "--partitions", "2"] + list(opts),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(tmp_path / out, "rb").read()

    want = run("want.ivf", "--yuv", str(tmp_path / "by_hand.yuv"), "--width", "64", "--height", "48")
    got = run("got.ivf", "--yuv", str(tmp_path / "surfaces.yuv"), "--surface", f"{SURFACE[0]}x{SURFACE[1]}", "--width", str(RAW[0]), "--height", str(RAW[1]),
              "--crop", f"{ORIGIN[0]}:{ORIGIN[1]}", "--rotate", "90")
    assert len(want) > 32 + 12 * FRAMES and got == want
