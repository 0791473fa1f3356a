"""The tools' -overlay option: scripts/native/y4m_to_ivf_gops -overlay ... writes, byte for byte, the file the one-video program
scripts/native/y4m_to_ivf -overlay ... writes -- with scene detection (an input with a cut) and without it, with one layer and with two,
at 64x48 and at a padded 60x44 -- the file is the one the serial program writes of the frames composed on the host, and without the
option both tools write the files they write of the plain frames."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlay_ref as R
from test_overlay_cpu import layer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, GOP, CUT = 13, 5, 7
COMMON = ["-g", str(GOP), "-partitions", "2"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("overlay_tools")
    exes = {}
    for name in ("y4m_to_ivf", "y4m_to_ivf_gops"):
        exes[name] = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", name + ".cpp"), "-o", exes[name],
                        "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    return exes


def video(W, H):
    """a moving synthetic picture with a cut at frame 7: another seed, U shifted by 45, and the chroma standing still between the cuts"""
    from vp8oclenc_amd.synth import SynthSequence
    seqs = [SynthSequence((W + 31) // 16 * 16, (H + 31) // 16 * 16, seed=5 + 31 * k) for k in range(2)]
    out = []
    for t in range(FRAMES):
        k = int(t >= CUT)
        y, (_, u, v) = seqs[k].frame(t)[0], seqs[k].frame(0)
        out.append((np.ascontiguousarray(y[:H, :W]), np.ascontiguousarray(np.clip(u[:H // 2, :W // 2].astype(int) + 45 * k, 0, 255).astype(np.uint8)),
                    np.ascontiguousarray(v[:H // 2, :W // 2])))
    return out


def run(*cmd):
    r = subprocess.run(list(cmd), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module", params=[(64, 48), (60, 44)], ids=["64x48", "60x44 padded"])
def case(request, tmp_path_factory):
    """the video, the same video with the two layers composed on the host, the layers' files and options"""
    from vp8oclenc_amd import y4m
    W, H = request.param
    d = tmp_path_factory.mktemp("case")
    frames = video(W, H)
    # a logo that reaches over the picture's last column and row (the padding behind it changes), and a band at a negative, odd position
    layers = [(layer(16, 16, "ramp", 21), W - 11, H - 9, 255), (layer(37, 21, "random", 22), -3, 11, 180)]
    options = []
    for k, (px, x, y, opacity) in enumerate(layers):
        px.tofile(str(d / f"layer{k}.bgra"))
        options.append(["-overlay", f"{d / f'layer{k}.bgra'}:{px.shape[1]}x{px.shape[0]}:{x}:{y}" + (f":{opacity}" if opacity != 255 else "")])
    y4m.write_y4m(str(d / "in.y4m"), frames, framerate=25)
    for n in (1, 2):
        burnt = [R.overlay_layers([(px, x, y, o, R.BGRA, 0) for px, x, y, o in layers[:n]], f) for f in frames]
        y4m.write_y4m(str(d / f"burnt{n}.y4m"), burnt, framerate=25)
    return d, options


@pytest.mark.parametrize("nlayers", [1, 2])
@pytest.mark.parametrize("scene", [False, True], ids=["no scene detection", "scene detection"])
def test_both_tools_write_the_file_of_the_composed_frames(programs, case, tmp_path, scene, nlayers):
    d, options = case
    overlay = [o for opt in options[:nlayers] for o in opt]
    serial_scene, gops_scene = ([], ["-scene-detect"]) if scene else (["-no-scene-detect"], [])
    run(programs["y4m_to_ivf"], str(d / "in.y4m"), str(tmp_path / "serial.ivf"), *COMMON, *serial_scene, *overlay)
    out = run(programs["y4m_to_ivf_gops"], str(d / "in.y4m"), str(tmp_path / "gops.ivf"), *COMMON, "-chunks", "3", "-batch", "2", *gops_scene, *overlay)
    run(programs["y4m_to_ivf"], str(d / f"burnt{nlayers}.y4m"), str(tmp_path / "burnt.ivf"), *COMMON, *serial_scene)
    one, many, burnt = (open(tmp_path / n, "rb").read() for n in ("serial.ivf", "gops.ivf", "burnt.ivf"))
    assert one == burnt, "y4m_to_ivf -overlay against y4m_to_ivf of the frames composed on the host"
    assert len(one) == len(many) and one == many, f"{len(one)} vs {len(many)} bytes, first difference at {next((i for i, (p, q) in enumerate(zip(one, many)) if p != q), None)}"
    if scene:
        assert "by scene change" in out, out


@pytest.mark.parametrize("scene", [False, True], ids=["no scene detection", "scene detection"])
def test_without_the_option_the_files_are_those_of_the_plain_frames(programs, case, tmp_path, scene):
    d, options = case
    serial_scene, gops_scene = ([], ["-scene-detect"]) if scene else (["-no-scene-detect"], [])
    run(programs["y4m_to_ivf"], str(d / "in.y4m"), str(tmp_path / "serial.ivf"), *COMMON, *serial_scene)
    run(programs["y4m_to_ivf_gops"], str(d / "in.y4m"), str(tmp_path / "gops.ivf"), *COMMON, "-chunks", "3", "-batch", "2", *gops_scene)
    # a layer at opacity 0 composes nothing: the bytes of the plain run, through the new launch
    faded = ["-overlay", options[0][1] + ":0"]
    run(programs["y4m_to_ivf"], str(d / "in.y4m"), str(tmp_path / "faded.ivf"), *COMMON, *serial_scene, *faded)
    run(programs["y4m_to_ivf"], str(d / "in.y4m"), str(tmp_path / "with.ivf"), *COMMON, *serial_scene, *options[0])
    one, many, faded_bytes, with_layer = (open(tmp_path / n, "rb").read() for n in ("serial.ivf", "gops.ivf", "faded.ivf", "with.ivf"))
    assert one == many and one == faded_bytes
    assert one != with_layer


def test_a_malformed_option_is_refused(programs, case, tmp_path):
    d, options = case
    for bad in ("nofile:16x16:0:0", options[0][1].split(":")[0] + ":17x16:0:0", options[0][1].split(":")[0] + ":16x16:0", options[0][1] + ":256"):
        for name in ("y4m_to_ivf", "y4m_to_ivf_gops"):
            r = subprocess.run([programs[name], str(d / "in.y4m"), str(tmp_path / "no.ivf"), "-overlay", bad], capture_output=True, text=True, timeout=300)
            assert r.returncode == 2 and "-overlay" in r.stderr, (name, bad, r.stdout + r.stderr)
