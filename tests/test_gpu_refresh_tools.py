"""Cyclic intra refresh in the tools: scripts/native/y4m_to_ivf -intra-refresh and scripts/encode_ivf.py --intra-refresh write the same
file, which is the stream the driver gives a caller and whose intra macroblocks are the rule's; the forced share is printed;
y4m_to_ivf_gops refuses the option; scripts/frame_bench.py runs with it."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import arf_ref
import refresh_ref as ref
from test_gpu_arf_tools import build, records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_tools_write_the_same_refreshed_file_and_its_intra_macroblocks_are_the_rules(tmp_path):
    import vp8_parse as vp
    from vp8oclenc_amd import api, y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    w, h, total, gop, P = 64, 48, 11, 7, 4
    mbw, mbh = w // 16, h // 16
    frames = arf_ref.noisy_pan(w, h, total, seed=w + total)
    y4m.write_y4m(str(tmp_path / "in.y4m"), frames, framerate=25)
    exe = build(tmp_path, "y4m_to_ivf")
    r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "native.ivf"), "-g", str(gop), "-intra-refresh", str(P), "-no-scene-detect", "-conformant",
                        "-qmin", "10", "-qmax", "60", "-partitions", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    phases = [t % gop - 1 for t in range(total) if t % gop]      # the phase restarts with every GOP
    forced = sum(api.intra_refresh_count(mbw, mbh, P, q) for q in phases)
    assert f"Intra refresh period {P}: {forced} of {total * mbw * mbh} macroblocks forced intra" in r.stderr, r.stderr
    common = ["--y4m", str(tmp_path / "in.y4m"), "--gop", str(gop), "--frames", str(total), "--intra-refresh", str(P), "--conformant", "--qmin", "10", "--qmax", "60",
              "--partitions", "2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "py.ivf")] + common, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "py.ivf", "rb").read() == open(tmp_path / "native.ivf", "rb").read()
    _, full = records(tmp_path / "native.ivf")
    st = vp.StreamState()
    for t, (_, b) in enumerate(full):
        f = vp.parse_frame(b, st)
        assert f.key == (t % gop == 0), t
        if not f.key:
            assert np.array_equal(f.is_inter == 0, ref.forced_map(mbw, mbh, P, t % gop - 1).reshape(-1)), t
    # what the tools refuse
    for bad in (["-intra-refresh", "3"], ["-intra-refresh", "1025"], ["-intra-refresh", "8", "-SSIM-target", "0.9"]):
        r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "bad.ivf")] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (bad, r.stdout + r.stderr)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "bad.ivf"), "--y4m", str(tmp_path / "in.y4m"), "--intra-refresh", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--intra-refresh" in r.stderr


def test_the_batched_tool_refuses_the_option(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = build(tmp_path, "y4m_to_ivf_gops")
    r = subprocess.run([exe, "in.y4m", "out.ivf", "-intra-refresh", "8"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "not batched" in r.stderr


def test_frame_bench_takes_the_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "frame_bench.py"), "--streams", "1", "--frames", "9", "--width", "64", "--height", "48",
                        "--intra-refresh", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "intra refresh, period 4:" in r.stdout and "k_intra_refresh (two wavefronts per forced macroblock) by HIP events" in r.stdout
