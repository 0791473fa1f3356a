"""Temporal layers in the tools: scripts/native/y4m_to_ivf -temporal-layers and scripts/encode_ivf.py --temporal-layers write the same
file, which is what the driver gives a caller; --keep-layers writes the frames of the lower layers with their own timestamps, and the RFC
6386 decoder of tests/vp8_decode.py takes that file; y4m_to_ivf_gops refuses the option; scripts/frame_bench.py runs with it."""
import os
import shutil
import subprocess
import sys

import pytest

import arf_ref
import temporal_ref as ref
from test_gpu_arf_tools import build, records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_tools_write_the_same_layered_file_and_its_base_layer_decodes(tmp_path):
    import vp8_decode
    from vp8oclenc_amd import api, y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    w, h, total, gop, layers = 64, 48, 13, 9, 3
    frames = arf_ref.noisy_pan(w, h, total, seed=w + total)
    y4m.write_y4m(str(tmp_path / "in.y4m"), frames, framerate=25)
    exe = build(tmp_path, "y4m_to_ivf")
    r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "native.ivf"), "-g", str(gop), "-temporal-layers", str(layers), "-no-check-ssim", "-no-scene-detect",
                        "-conformant", "-qmin", "10", "-qmax", "60", "-partitions", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ref.records(layers, {gop}, total)
    tids = [x["temporal_id"] for x in want]
    per_layer = " / ".join(str(tids.count(k)) for k in range(3))
    unfiltered = sum(x["refresh"] == ref.NONE for x in want)
    assert f"frames in layer 0 / 1 / 2: {per_layer}; {unfiltered} unreferenced frames not loop-filtered" in r.stdout, r.stdout
    common = ["--y4m", str(tmp_path / "in.y4m"), "--gop", str(gop), "--frames", str(total), "--temporal-layers", str(layers), "--no-check-ssim", "--conformant",
              "--qmin", "10", "--qmax", "60", "--partitions", "2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "py.ivf")] + common, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "py.ivf", "rb").read() == open(tmp_path / "native.ivf", "rb").read()
    assert f"frames in layer 0 / 1 / 2: {per_layer}" in r.stdout
    # ... and it is the stream the driver gives a caller
    drv = api.NativeDriver(w, h, gop_size=gop, altref_range=gop + 1, check_ssim=0, conformant_stream=1, qi_min=10, qi_max=60, num_partitions=2)
    drv.set_temporal_layers(layers)
    count, full = records(tmp_path / "native.ivf")
    assert count == total + 1 and [ts for ts, _ in full] == list(range(total))
    for t, f in enumerate(frames):
        drv.encode_frame_host(*f)
        assert drv.get_frame() == full[t][1], t
        assert drv.frame_layer().temporal_id == tids[t]
    drv.close()
    # --keep-layers K: the frames of temporal_id <= K of that file, their own timestamps, the count of the frames written
    dec = vp8_decode.Decoder()
    pictures = [dec.decode(b)[1] for _, b in full]
    for K in (1, 0):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / f"keep{K}.ivf")] + common + ["--keep-layers", str(K)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        count, kept = records(tmp_path / f"keep{K}.ivf")
        assert kept == [full[t] for t in range(total) if tids[t] <= K] and count == len(kept) < total
        dec = vp8_decode.Decoder()
        for ts, b in kept:
            _, planes = dec.decode(b)
            assert all((a == p).all() for a, p in zip(planes, pictures[ts])), (K, ts)
    # what the tools refuse
    for bad in (["-temporal-layers", "4"], ["-temporal-layers", "0"], ["-temporal-layers", "2", "-arf", "4"]):
        r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "bad.ivf")] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (bad, r.stdout + r.stderr)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "bad.ivf"), "--y4m", str(tmp_path / "in.y4m"), "--keep-layers", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--temporal-layers" in r.stderr


def test_the_batched_tool_refuses_the_option(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = build(tmp_path, "y4m_to_ivf_gops")
    r = subprocess.run([exe, "in.y4m", "out.ivf", "-temporal-layers", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "not batched" in r.stderr


def test_frame_bench_takes_the_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "frame_bench.py"), "--streams", "1", "--frames", "9", "--width", "64", "--height", "48",
                        "--temporal-layers", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "temporal layers 3: of every 4 inter frames 2 refresh no buffer and 1 search GOLDEN beside LAST" in r.stdout and "not loop-filtered" in r.stdout
