"""Quality statistics of the coded frames (vp8hip_set_quality_stats, vp8drv_config.quality_stats): the metric restated in numpy, the
ABI of its structs, and the kernel's register budget (no GPU needed)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = 26634, 239708


def psnr(sse, samples):
    return 100.0 if sse == 0 else 10.0 * np.log10(samples * 255.0 ** 2 / sse)


def plane_stats(s, r):
    """(sse, samples, ssim) of one plane's region: libvpx's integer SSIM, 8x8 windows every 4 samples"""
    s, r = s.astype(np.int64), r.astype(np.int64)
    sse = int(((s - r) ** 2).sum())
    h, w = s.shape
    fbr, fbc = h // 4, w // 4
    if fbr < 2 or fbc < 2:
        return sse, w * h, (1.0 if sse == 0 else 0.0)
    blocks = [x[:fbr * 4, :fbc * 4].reshape(fbr, 4, fbc, 4).sum(axis=(1, 3)) for x in (s, r, s * s, r * r, s * r)]
    S, R, SS, RR, SR = (b[:-1, :-1] + b[1:, :-1] + b[:-1, 1:] + b[1:, 1:] for b in blocks)
    num = (2 * S * R + C1) * (128 * SR - 2 * S * R + C2)
    den = (S * S + R * R + C1) * (64 * SS - S * S + 64 * RR - R * R + C2)
    return sse, w * h, float(np.mean(num.astype(np.float64) / den.astype(np.float64)))


def frame_stats(src, rec, w, h):
    """the record of one frame: src, rec = (Y, U, V) planes at least as large as the region (w x h luma)"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    regions = [(h, w), (ch, cw), (ch, cw)]
    st = [plane_stats(s[:y, :x], r[:y, :x]) for s, r, (y, x) in zip(src, rec, regions)]
    sse, n, ssim = [x[0] for x in st], [x[1] for x in st], [x[2] for x in st]
    return dict(sse=sse, samples=n, psnr=[psnr(a, b) for a, b in zip(sse, n)], psnr_all=psnr(sum(sse), sum(n)), ssim=ssim,
                ssim_all=0.8 * ssim[0] + 0.1 * (ssim[1] + ssim[2]))


def planes(w, h, f):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return f((h, w)), f((ch, cw)), f((ch, cw))


def test_identical_planes_give_100_db_and_ssim_1():
    rng = np.random.default_rng(1)
    src = planes(64, 48, lambda shp: rng.integers(0, 256, shp, dtype=np.uint8))
    r = frame_stats(src, src, 64, 48)
    assert r["sse"] == [0, 0, 0] and r["psnr"] == [100.0] * 3 and r["psnr_all"] == 100.0
    assert r["ssim"] == [1.0, 1.0, 1.0] and r["ssim_all"] == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("d", [1, 7, 40])
def test_a_constant_offset_gives_the_closed_form_psnr(d):
    rng = np.random.default_rng(d)
    src = planes(40, 24, lambda shp: rng.integers(0, 200, shp, dtype=np.uint8))
    rec = [(p + d).astype(np.uint8) for p in src]
    r = frame_stats(src, rec, 40, 24)
    n = [40 * 24, 20 * 12, 20 * 12]
    assert r["sse"] == [k * d * d for k in n] and r["samples"] == n
    want = 10 * np.log10(255.0 ** 2 / d ** 2)
    assert r["psnr"] == pytest.approx([want] * 3, rel=1e-12) and r["psnr_all"] == pytest.approx(want, rel=1e-12)
    assert all(0 < s < 1 for s in r["ssim"])


def test_a_17x9_source_has_no_whole_chroma_window():
    rng = np.random.default_rng(3)
    src = planes(17, 9, lambda shp: rng.integers(0, 256, shp, dtype=np.uint8))
    rec = [p.copy() for p in src]
    rec[1][0, 0] ^= 1
    r = frame_stats(src, rec, 17, 9)
    assert r["samples"] == [153, 45, 45]
    assert r["ssim"][1] == 0.0 and r["ssim"][2] == 1.0   # chroma 9x5: no whole window; sse decides
    assert r["ssim"][0] == 1.0                           # luma 17x9: 3 x 1 windows, identical
    # the window sums equal sums over the 8x8 windows themselves
    s = rng.integers(0, 256, (16, 16)).astype(np.int64)
    t = rng.integers(0, 256, (16, 16)).astype(np.int64)
    got = plane_stats(s.astype(np.uint8), t.astype(np.uint8))[2]
    vals = []
    for i in range(0, 9, 4):
        for j in range(0, 9, 4):
            a, b = s[i:i + 8, j:j + 8], t[i:i + 8, j:j + 8]
            S, R, SS, RR, SR = a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()
            vals.append((2 * S * R + C1) * (128 * SR - 2 * S * R + C2) / ((S * S + R * R + C1) * (64 * SS - S * S + 64 * RR - R * R + C2)))
    assert got == pytest.approx(np.mean(vals), rel=1e-12)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_quality_structs_have_the_c_layout(tmp_path):
    src = tmp_path / "l.c"
    src.write_text("""
        #include <stdio.h>
        #include <stddef.h>
        #include "vp8hip_driver.h"
        int main(void) {
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(vp8drv_quality), offsetof(vp8drv_quality, sse),
                   offsetof(vp8drv_quality, psnr_all), offsetof(vp8drv_quality, ssim_all), sizeof(vp8drv_quality_summary),
                   offsetof(vp8drv_quality_summary, psnr_avg), offsetof(vp8drv_quality_summary, psnr_min_frame),
                   sizeof(vp8drv_config), offsetof(vp8drv_config, quality_stats), offsetof(vp8drv_config, loop_filter_type));
            return 0;
        }
    """)
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Q, S, D = api.Quality, api.QualitySummary, api.DrvConfig
    assert c[:4] == [C.sizeof(Q), Q.sse.offset, Q.psnr_all.offset, Q.ssim_all.offset]
    assert c[4:7] == [C.sizeof(S), S.psnr_avg.offset, S.psnr_min_frame.offset]
    assert c[7:] == [C.sizeof(D), D.quality_stats.offset, D.loop_filter_type.offset]
    assert D.quality_stats.offset == C.sizeof(D) - 4     # the last field


def test_default_config_has_stats_off_and_the_abi_version_is_4010():
    lib = api.load_library()
    cfg = api.DrvConfig()
    cfg.quality_stats = 7
    lib.vp8drv_default_config.argtypes = [C.POINTER(api.DrvConfig)]
    lib.vp8drv_default_config.restype = None
    lib.vp8drv_default_config(C.byref(cfg))
    assert cfg.quality_stats == 0
    assert api.ABI_VERSION == 4010 and lib.vp8hip_abi_version() == 4010
    text = open(os.path.join(ROOT, "include", "vp8hip.h")).read()
    assert re.search(r"#define VP8HIP_ABI_VERSION 4010\b", text)
    for name in ("vp8hip_set_quality_stats", "vp8hip_quality_result", "vp8hip_quality_summary", "vp8hip_batch_quality",
                 "vp8drv_get_frame_quality", "vp8drv_get_quality_summary", "vp8hip_debug_quality"):
        assert hasattr(lib, name), name


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_quality_kernels_use_no_scratch_and_stay_inside_their_register_budget(tmp_path):
    out = tmp_path / "k.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(ROOT, "vp8oclenc_amd", "csrc", "kernels_quality.hip"), "-o", str(out), "-w"],
                   check=True, timeout=600)
    text = out.read_text()
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:.*\n)*?)\s+\.wavefront_size", text):
        name, body = m.group(1), m.group(2)
        for frag in ("k_quality", "k_quality_b"):
            if re.search(frag + r"E", name):
                seen.add(frag)
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
                vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
                spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
                assert scratch == 0 and spills == 0, f"{name}: {scratch} B of scratch, {spills} spilled VGPRs"
                assert vgprs <= 96, f"{name}: {vgprs} VGPRs (budget 96: five waves per SIMD)"
    assert seen == {"k_quality", "k_quality_b"}, seen
