"""Frame analysis statistics without a GPU: vp8host_analyse_luma (the source-side rule in plain C++) against the numpy restatement of
tests/analysis_ref.py, the record's layout against a C compiler's, and an ABI that only grew.  Everything is exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import analysis_ref as ref
from vp8oclenc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(16, 16), (48, 32), (176, 144)]
NEW_SYMBOLS = ["vp8hip_set_analysis", "vp8hip_analysis_restart", "vp8hip_analysis_result", "vp8host_analyse_luma", "vp8drv_set_analysis",
               "vp8drv_get_frame_analysis", "vp8drv_set_quantizer", "vp8drv_get_quantizer"]


@pytest.mark.parametrize("w,h", SIZES)
def test_host_rule_equals_the_restatement(w, h):
    a, b = ref.planes(w, h, "random", 1), ref.planes(w, h, "random", 2)
    assert api.analyse_luma(a, b) == ref.source_side(a, b)
    assert api.analyse_luma(b, a) == ref.source_side(b, a)
    e0, e1 = ref.planes(w, h, "extremes", 3), ref.planes(w, h, "extremes", 4)      # the widest sums
    assert api.analyse_luma(e0, e1) == ref.source_side(e0, e1)
    assert api.analyse_luma(e0, 255 - e0)["temporal_sse"] == w * h * 255 * 255


@pytest.mark.parametrize("w,h", SIZES)
def test_constant_static_single_sample_and_no_history(w, h):
    mbs = (w // 16) * (h // 16)
    c, r = ref.planes(w, h, "constant"), ref.planes(w, h, "random", 5)
    got = api.analyse_luma(c, r)
    assert got == ref.source_side(c, r) and got["spatial"] == 0 and got["have_prev"] == 1
    got = api.analyse_luma(r, r.copy())      # cur == prev: every macroblock static
    assert got == ref.source_side(r, r) and (got["static_mbs"], got["temporal_sse"], got["temporal_sad"]) == (mbs, 0, 0)
    one = np.zeros((h, w), np.uint8)
    one[h - 1, w - 1] = 255                  # one sample differing by 255: SSE 65025, SAD 255, one macroblock not static
    got = api.analyse_luma(one, np.zeros((h, w), np.uint8))
    assert got == ref.source_side(one, np.zeros((h, w), np.uint8))
    assert (got["temporal_sse"], got["temporal_sad"], got["static_mbs"]) == (65025, 255, mbs - 1)
    assert got["spatial"] == 256 * 65025 - 65025
    got = api.analyse_luma(r)                # prev = NULL
    assert got == ref.source_side(r, None)
    assert (got["have_prev"], got["temporal_sse"], got["temporal_sad"], got["static_mbs"]) == (0, 0, 0, 0) and got["spatial"] > 0


def test_bad_arguments_are_refused():
    lib = api.load_library()
    lib.vp8host_analyse_luma.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.vp8host_analyse_luma.restype = C.c_int
    p = np.zeros((32, 32), np.uint8)
    out = api.LumaAnalysis()
    assert lib.vp8host_analyse_luma(p.ctypes.data, None, 32, 32, C.byref(out)) == 0
    assert lib.vp8host_analyse_luma(None, None, 32, 32, C.byref(out)) == -1
    assert lib.vp8host_analyse_luma(p.ctypes.data, None, 32, 32, None) == -1
    for w, h in ((24, 32), (32, 24), (0, 32), (32, 0), (8, 8), (-16, 16)):      # not whole macroblocks, or none at all
        assert lib.vp8host_analyse_luma(p.ctypes.data, p.ctypes.data, w, h, C.byref(out)) == -1, (w, h)
    with pytest.raises(ValueError):
        api.analyse_luma(p[:, :24])
    with pytest.raises(ValueError):
        api.analyse_luma(p, p[:16])


def test_record_layout_against_the_headers(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [n for n, _ in api.Analysis._fields_]
    host = [n for n, _ in api.LumaAnalysis._fields_]
    src = tmp_path / "s.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"vp8hip_driver.h\"\n#include \"vp8hip_host.h\"\nint main(void) {\n"
                   "printf(\"%zu %zu %zu\\n\", sizeof(vp8hip_analysis), sizeof(vp8drv_analysis), sizeof(vp8host_luma_analysis));\n" +
                   "".join(f"printf(\"%zu\\n\", offsetof(vp8hip_analysis, {n}));\n" for n in names) +
                   "".join(f"printf(\"%zu\\n\", offsetof(vp8host_luma_analysis, {n}));\n" for n in host) +
                   "printf(\"%zu %zu\\n\", sizeof(vp8drv_config), offsetof(vp8drv_config, quality_stats));\nreturn 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert c[0] == c[1] == C.sizeof(api.Analysis) == 144
    assert c[2] == C.sizeof(api.LumaAnalysis) == 32
    assert c[3:3 + len(names)] == [getattr(api.Analysis, n).offset for n in names]
    assert c[3 + len(names):3 + len(names) + len(host)] == [getattr(api.LumaAnalysis, n).offset for n in host]
    assert c[-2:] == [C.sizeof(api.DrvConfig), api.DrvConfig.quality_stats.offset] == [88, 84]
    # every field the rule names is in the struct, and no float is
    hdr = open(os.path.join(ROOT, "include", "vp8hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} vp8hip_analysis;", hdr).group(1)
    assert not re.search(r"\b(float|double)\b", body)
    for f in ref.SOURCE_FIELDS + ref.CODING_FIELDS + ("frame_number", "is_key"):
        assert re.search(r"\b" + f + r"\b", body), f
        assert f in names
    assert api.Analysis.SOURCE_FIELDS == ref.SOURCE_FIELDS and api.Analysis.CODING_FIELDS == ref.CODING_FIELDS


def test_abi_new_entry_points_and_nothing_else_moved():
    lib = api.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in api.ABI_SYMBOLS, name
    lib.vp8hip_abi_version.restype = C.c_int
    assert lib.vp8hip_abi_version() == 4010 == api.ABI_VERSION
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("vp8hip.h", "vp8hip_driver.h", "vp8hip_host.h"))
    assert int(re.search(r"#define VP8HIP_ABI_VERSION (\d+)", hdr).group(1)) == 4010
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    # vp8drv_config and its defaults are what they were: the new switches are entry points
    assert C.sizeof(api.DrvConfig) == 88 and api.DrvConfig._fields_[-1][0] == "quality_stats"
    lib.vp8drv_default_config.argtypes = [C.POINTER(api.DrvConfig)]
    lib.vp8drv_default_config.restype = None
    cfg = api.DrvConfig()
    C.memset(C.byref(cfg), 0xff, C.sizeof(cfg))
    lib.vp8drv_default_config(C.byref(cfg))
    want = dict(gop_size=150, altref_range=5, qi_min=0, qi_max=48, device_params=1, check_ssim=1, num_partitions=1, display_width=0,
                display_height=0, host_bitstream=0, overlap_filter=0, ref_mask=3, conformant_stream=0, scene_detect=0, src_width=0,
                src_height=0, loop_filter_type=0, in_width=0, in_height=0, scale_filter=0, quality_stats=0)
    assert {k: getattr(cfg, k) for k in want} == want and cfg.ssim_target == -1.0
    assert sorted(list(want) + ["ssim_target"]) == sorted(n for n, _ in api.DrvConfig._fields_)      # (every field was looked at)


def test_text_line_carries_every_field():
    a = api.Analysis()
    a.frame_number, a.is_key, a.spatial, a.mv_sum[1], a.segment_mbs[3] = 7, 1, 2 ** 40, -5, 9
    words = a.text_line(1234).split(" ")
    assert words[:3] == ["7", "1", "1234"]
    assert len(words) == 3 + 5 + 6 + 3 + 4 + 2 + 2 + 2      # source side; coded + five counts; mbs_ref; segment_mbs; the mv sums; sq + nz
    assert str(2 ** 40) in words and "-5" in words and "9" in words
