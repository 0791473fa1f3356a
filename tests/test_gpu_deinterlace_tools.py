"""The native tools' -deinterlace option (scripts/native/y4m_to_ivf.cpp, y4m_to_ivf_gops.cpp): an interlaced Y4M file coded frame after
frame and with its closed GOPs side by side gives one file, the Python driver's frames; the field kept comes from the header's I tag;
an Im file is refused; without the option nothing changes, whatever the tag says."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import deinterlace_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_y4m(path, frames, tag):
    h, w = frames[0][0].shape
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F25:1 {tag + ' ' if tag else ''}A1:1 C420jpeg\n".encode())
        for planes in frames:
            f.write(b"FRAME\n")
            for p in planes:
                f.write(np.ascontiguousarray(p).tobytes())


def ivf_frames(data):
    out, at = [], 32
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], "little")
        out.append(data[at + 12:at + 12 + n])
        at += 12 + n
    return out


def test_the_two_programs_write_one_file_and_the_python_drivers_frames(tmp_path):
    from vp8oclenc_amd import api
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exes = {}
    for name in ("y4m_to_ivf", "y4m_to_ivf_gops"):
        exes[name] = str(tmp_path / name)
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", name + ".cpp"), "-o", exes[name],
                        "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    W, H, n = 64, 48, 8
    frames = ref.interlaced_video(W, H, n, seed=6)
    for tag in ("It", "Ib", "", "Im"):
        write_y4m(str(tmp_path / f"{tag or 'none'}.y4m"), frames, tag)

    def run(name, src, out, *opts, ok=True):
        cmd = [exes[name], str(tmp_path / src), str(tmp_path / out), "-g", "4"] + (["-no-scene-detect"] if name == "y4m_to_ivf" else ["-chunks", "2", "-batch", "2"]) + list(opts)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return r.stderr if not ok else (open(tmp_path / out, "rb").read(), r.stderr)

    def driver(mode, keep):
        drv = api.NativeDriver(W, H, gop_size=4)
        if mode:
            drv.set_deinterlace(mode, keep)
        out = []
        for f in frames:
            drv.encode_frame_host(*f)
            out.append(drv.get_frame())
        drv.close()
        return out

    serial, err = run("y4m_to_ivf", "It.y4m", "serial.ivf", "-deinterlace", "adaptive")
    gops, _ = run("y4m_to_ivf_gops", "It.y4m", "gops.ivf", "-deinterlace", "adaptive")
    assert serial == gops
    top = driver(2, 0)
    assert ivf_frames(serial) == top
    assert "woven" in err and "top field kept" in err
    # the field kept: the first field of the tag, or the one named; top, and a line on stderr, for a file that names no field order
    bottom = driver(2, 1)
    assert top != bottom
    assert ivf_frames(run("y4m_to_ivf", "Ib.y4m", "b.ivf", "-deinterlace", "adaptive")[0]) == bottom
    assert ivf_frames(run("y4m_to_ivf_gops", "Ib.y4m", "bt.ivf", "-deinterlace", "adaptive:top")[0]) == top
    data, err = run("y4m_to_ivf", "none.y4m", "p.ivf", "-deinterlace", "adaptive")
    assert ivf_frames(data) == top and "keeps the top field" in err
    for name in exes:      # (refused when the header is read: nothing is coded)
        assert "Im" in run(name, "Im.y4m", "no.ivf", "-deinterlace", "adaptive", ok=False)
    # without the option: what the tools write today for this file, whatever the tag says
    plain = driver(0, 0)
    assert plain != top
    for name, src in (("y4m_to_ivf", "It.y4m"), ("y4m_to_ivf_gops", "It.y4m"), ("y4m_to_ivf", "Im.y4m")):
        assert ivf_frames(run(name, src, "plain.ivf")[0]) == plain, (name, src)
