"""The native tool's -arf option (scripts/native/y4m_to_ivf.cpp): a Y4M file coded with hidden alternate reference frames is, record for
record, what the driver gives a caller that hands in the same windows (tests/arf_ref.schedule is the placement both follow); a hidden
frame is a record of its own with the timestamp of the next shown frame, the header's frame count includes it, and the file decodes
with the RFC 6386 decoder of tests/vp8_decode.py.  scripts/encode_ivf.py --arf writes the same file; scripts/frame_bench.py --arf runs;
y4m_to_ivf_gops refuses the option."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import arf_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "native", name + ".cpp"), "-o", exe,
                    "-L", os.path.join(ROOT, "vp8oclenc_amd"), "-lvp8hip", "-Wl,-rpath," + os.path.join(ROOT, "vp8oclenc_amd")], check=True, timeout=300)
    return exe


def records(path):
    data = open(path, "rb").read()
    assert data[:4] == b"DKIF"
    count, = struct.unpack_from("<I", data, 24)
    out, at = [], 32
    while at < len(data):
        size, ts = struct.unpack_from("<IQ", data, at)
        out.append((ts, data[at + 12:at + 12 + size]))
        at += 12 + size
    return count, out


def test_the_native_tool_codes_the_hidden_frames_a_caller_of_the_driver_codes(tmp_path):
    import vp8_decode
    from vp8oclenc_amd import api, y4m
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    w, h, total, gop, period, nmax, strength = 64, 48, 14, 9, 4, 5, 2
    frames = ref.noisy_pan(w, h, total, seed=12)
    y4m.write_y4m(str(tmp_path / "in.y4m"), frames, framerate=25)
    exe = build(tmp_path, "y4m_to_ivf")
    r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "arf.ivf"), "-g", str(gop), "-arf", f"{period}:{nmax}:{strength}", "-conformant", "-qmin", "10",
                        "-qmax", "60", "-partitions", "2", "-psnr", "-no-scene-detect"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    placement = ref.schedule(total, gop, period, nmax)
    assert sorted(placement) == [0, 4, 8, 9, 13]
    drv = api.NativeDriver(w, h, gop_size=gop, conformant_stream=1, qi_min=10, qi_max=60, num_partitions=2, quality_stats=1)
    drv.set_arf(strength + 1)
    want = []
    for ev in ref.events(total, placement):
        if ev[0] == "hidden":
            _, t, lo, n, centre = ev
            drv.encode_arf_host(frames[lo:lo + n], centre)
            want.append((t + (placement[t][3] == "after"), drv.get_frame()))      # the timestamp of the next shown frame
        else:
            drv.encode_frame_host(*frames[ev[1]])
            want.append((ev[1], drv.get_frame()))
            drv.resolve()
    drv.close()
    count, got = records(tmp_path / "arf.ivf")
    assert count == len(got) + 1 == total + len(placement) + 1      # (one more than the file holds, as without the option; the hidden frames included)
    assert [ts for ts, _ in got] == [ts for ts, _ in want]
    for i, ((_, a), (_, b)) in enumerate(zip(got, want)):
        assert a == b, f"record {i}: {len(a)} bytes for {len(b)}"
    assert f"{len(placement)} hidden" in r.stdout and "Hidden alt-refs: 5" in r.stderr and "(14 frames)" in r.stderr      # -psnr counts the shown frames
    dec = vp8_decode.Decoder()
    shown = 0
    for ts, b in got:
        f, planes = dec.decode(b)
        shown += f.show
        assert f.show or (f.refresh_last, f.refresh_altref) == (0, 1)
    assert shown == total
    # with scene detection, the tool's default, the option still runs and every shown frame is there (where the detector puts key frames
    # is the content's business: tests/test_gpu_arf.py holds it to the run without hidden frames)
    common = ["-g", str(gop), "-arf", f"{period}:{nmax}:{strength}", "-conformant", "-qmin", "10", "-qmax", "60", "-partitions", "2"]
    r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "arf_sd.ivf")] + common, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{total} shown" in r.stdout, r.stdout + r.stderr
    dec = vp8_decode.Decoder()
    assert sum(dec.decode(b)[0].show for _, b in records(tmp_path / "arf_sd.ivf")[1]) == total
    # scripts/encode_ivf.py --arf writes the file the tool writes with -no-scene-detect
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "py.ivf"), "--y4m", str(tmp_path / "in.y4m"), "--gop", str(gop),
                        "--frames", str(total), "--arf", f"{period}:{nmax}:{strength}", "--conformant", "--qmin", "10", "--qmax", "60", "--partitions", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "py.ivf", "rb").read() == open(tmp_path / "arf.ivf", "rb").read()
    assert f"{len(placement)} hidden" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "encode_ivf.py"), str(tmp_path / "bad.ivf"), "--y4m", str(tmp_path / "in.y4m"), "--arf", "4:9"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "FRAMES 1..7" in r.stderr
    # without the option the file is the one it was: no record is hidden
    r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "plain.ivf"), "-g", str(gop)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    count, got = records(tmp_path / "plain.ivf")
    assert count == total + 1 and all(b[0] & 0x10 for _, b in got)
    for bad in (["-arf", "0"], ["-arf", "4:8"], ["-arf", "4:7:7"], ["-arf", "4", "-denoise", "1"]):
        r = subprocess.run([exe, str(tmp_path / "in.y4m"), str(tmp_path / "bad.ivf")] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (bad, r.stdout + r.stderr)


def test_the_batched_tool_refuses_the_option(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = build(tmp_path, "y4m_to_ivf_gops")
    r = subprocess.run([exe, "in.y4m", "out.ivf", "-arf", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "not batched" in r.stderr


def test_frame_bench_takes_the_option():
    """scripts/frame_bench.py --arf: every stream codes hidden frames from device-resident windows; with one stream it also times the filter"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "frame_bench.py"), "--streams", "1", "--frames", "9", "--width", "64", "--height", "48",
                        "--arf", "4:5:2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hidden alt-refs (--arf 4:5:2)" in r.stdout and "5 frames" in r.stdout and "k_arf_filter_b, window of 5" in r.stdout
