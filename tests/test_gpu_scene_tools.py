"""Scene cuts in the GOP-parallel tools: scripts/native/y4m_to_ivf_gops -scene-detect and scripts/encode_ivf.py --scene-detect write, byte
for byte, the file the one-video program scripts/native/y4m_to_ivf writes with ITS default (scene detection on).  The video is the
constructed case of tests/test_scene_plan_cpu.py: g = 9, 34 frames, cuts at 6, 8, 21, 22 and 33, key frames at 0, 6, 12, 21, 26, 33 --
a hold-over key frame, a cut on a scheduled key frame that is never looked at, a deferred cut, a last chunk of one frame."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_scene_plan_cpu import CONSTRUCTED_CUTS, CONSTRUCTED_KEYS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, GOP = 34, 9


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("scene_tools")
    exes = {}
    for name in ("y4m_to_ivf", "y4m_to_ivf_gops"):
        exes[name] = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", name + ".cpp"), "-o", exes[name],
                        "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    return exes


def write_video(path, W, H, cuts=CONSTRUCTED_CUTS, frames=FRAMES):
    """the synthetic sequence cut out of a larger one, another seed and U shifted by 45 behind every cut (as tests/test_gpu_file_roundtrip.py
    makes its cut)"""
    from vp8oclenc_amd import y4m
    from vp8oclenc_amd.synth import SynthSequence
    seqs = [SynthSequence((W + 31) // 16 * 16, (H + 31) // 16 * 16, seed=3 + 29 * k) for k in range(len(cuts) + 1)]
    src = []
    for t in range(frames):
        k = sum(t >= c for c in cuts)
        y, u, v = seqs[k].frame(t)
        src.append((np.ascontiguousarray(y[:H, :W]), np.ascontiguousarray(np.clip(u[:H // 2, :W // 2].astype(int) + 45 * (k & 1), 0, 255).astype(np.uint8)),
                    np.ascontiguousarray(v[:H // 2, :W // 2])))
    y4m.write_y4m(str(path), src, framerate=25)


def run(*cmd):
    r = subprocess.run(list(cmd), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def key_frames_of(path):
    import decode_ivf
    return [t for t, p in enumerate(decode_ivf.read_ivf(str(path))[4]) if not (p[0] & 1)]


sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module", params=[(360, 200, []), (354, 290, ["-resize", "240x196"])], ids=["360x200", "354x290 resized"])
def serial_file(request, programs, tmp_path_factory):
    """the video and the serial program's file of it, once per size: (in.y4m, serial.ivf, its key and scene-change counts, the options)"""
    W, H, extra = request.param
    d = tmp_path_factory.mktemp("serial")
    write_video(d / "in.y4m", W, H)
    out = run(programs["y4m_to_ivf"], str(d / "in.y4m"), str(d / "serial.ivf"), "-g", str(GOP), "-partitions", "2", *extra)
    m = re.search(r"(\d+) key \((\d+) by scene change", out)
    assert m, out
    assert key_frames_of(d / "serial.ivf") == CONSTRUCTED_KEYS      # the serial program, by the rule
    return d / "in.y4m", d / "serial.ivf", (int(m.group(1)), int(m.group(2))), extra


@pytest.mark.parametrize("chunks,batch", [(5, 3), (48, 6), (2, 1)])
def test_the_batched_program_with_scene_detection_writes_the_serial_programs_file(programs, serial_file, tmp_path, chunks, batch):
    src, serial, counts, extra = serial_file
    out = run(programs["y4m_to_ivf_gops"], str(src), str(tmp_path / "gops.ivf"), "-g", str(GOP), "-partitions", "2", "-scene-detect", "-chunks", str(chunks), "-batch", str(batch), *extra)
    m = re.search(r"scene plan: (\d+) key \((\d+) by scene change\), (\d+) chunks", out)
    assert m, out
    assert (int(m.group(1)), int(m.group(2))) == counts == (6, 4) and int(m.group(3)) == 6, out
    assert f"{counts[0]} key frames" in out, out      # ... and as many were coded
    one, many = open(serial, "rb").read(), open(tmp_path / "gops.ivf", "rb").read()
    assert len(one) == len(many) and one == many, f"{len(one)} vs {len(many)} bytes, first difference at {next((i for i, (p, q) in enumerate(zip(one, many)) if p != q), None)}"


def test_a_file_without_cuts_is_the_same_with_and_without_the_option(programs, tmp_path):
    write_video(tmp_path / "in.y4m", 320, 192, cuts=(), frames=23)
    common = [str(tmp_path / "in.y4m")], ["-g", "5", "-chunks", "3", "-batch", "2"]
    plain = run(programs["y4m_to_ivf_gops"], *common[0], str(tmp_path / "a.ivf"), *common[1])
    scene = run(programs["y4m_to_ivf_gops"], *common[0], str(tmp_path / "b.ivf"), *common[1], "-scene-detect")
    assert "scene plan" not in plain and "scene plan: 5 key (0 by scene change), 5 chunks" in scene, plain + scene
    assert open(tmp_path / "a.ivf", "rb").read() == open(tmp_path / "b.ivf", "rb").read()
    assert plain.splitlines()[0] == scene.splitlines()[0].replace("b.ivf", "a.ivf")      # the summary line says the same


@pytest.mark.parametrize("extra", [["-denoise", "2"], ["-deinterlace", "adaptive"], ["-deinterlace", "adaptive:bottom"]])
def test_the_two_refusals(programs, tmp_path, extra):
    write_video(tmp_path / "in.y4m", 64, 48, cuts=(), frames=2)
    r = subprocess.run([programs["y4m_to_ivf_gops"], str(tmp_path / "in.y4m"), str(tmp_path / "out.ivf"), "-scene-detect", *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "-scene-detect with" in r.stderr and not os.path.exists(tmp_path / "out.ivf"), r.stdout + r.stderr


def test_encode_ivf_with_scene_detection_writes_the_serial_programs_file(serial_file, tmp_path):
    src, serial, counts, extra = serial_file
    args = ["--resize", extra[1]] if extra else []
    out = run(sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "py.ivf"), "--y4m", str(src), "--frames", str(FRAMES), "--gop", str(GOP),
              "--partitions", "2", "--scene-detect", "--scan-batch", "3", *args)
    assert f"scene plan: {counts[0]} key ({counts[1]} by scene change)" in out, out
    assert open(serial, "rb").read() == open(tmp_path / "py.ivf", "rb").read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "no.ivf"), "--y4m", str(src), "--scene-detect", "--denoise", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--scene-detect does not go with" in r.stderr
