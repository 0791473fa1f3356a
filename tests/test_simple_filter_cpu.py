"""The simple loop filter (vp8hip_set_loop_filter_type 1) without a GPU: the ABI that carries it, the gfx950 code of its kernels,
and the RFC 6386 section 15.2 restatement (tests/vp8_decode_simple.py) held to libwebp on key frames coded with filter_type 1."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import webp_decode
from vp8_decode_simple import simple_filter_plane
from vp8oclenc_amd import api
from vp8oclenc_amd.synth import SynthSequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_loop_filter_type_is_exported():
    assert "vp8hip_set_loop_filter_type" in api.ABI_SYMBOLS
    assert hasattr(api.load_library(), "vp8hip_set_loop_filter_type")


def test_driver_config_carries_loop_filter_type_at_the_c_offset(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "s.c"
    src.write_text("""
        #include <stdio.h>
        #include <stddef.h>
        #include "vp8hip_driver.h"
        int main(void) {
            vp8drv_config c;
            printf("%zu %zu\\n", sizeof(vp8drv_config), offsetof(vp8drv_config, loop_filter_type));
            return 0;
        }""")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert size == C.sizeof(api.DrvConfig) and off == api.DrvConfig.loop_filter_type.offset
    lib = api.load_library()
    cfg = api.DrvConfig()
    cfg.loop_filter_type = 7
    lib.vp8drv_default_config.argtypes = [C.POINTER(api.DrvConfig)]
    lib.vp8drv_default_config.restype = None
    lib.vp8drv_default_config(C.byref(cfg))
    assert cfg.loop_filter_type == 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_simple_filter_kernels_use_no_scratch_and_stay_inside_their_register_budget(tmp_path):
    out = tmp_path / "k.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                    "--cuda-device-only", "-S", os.path.join(ROOT, "vp8oclenc_amd", "csrc", "kernels_lf_simple.hip"), "-o", str(out), "-w"],
                   check=True, timeout=600)
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:.*\n)*?)\s+\.wavefront_size", out.read_text()):
        name, body = m.group(1), m.group(2)
        for frag in ("k_loop_filter_simpleENS", "k_loop_filter_simple_bENS"):
            if frag in name:
                seen.add(frag)
                scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1))
                vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", body).group(1))
                spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", body).group(1))
                assert scratch == 0 and spills == 0, f"{name}: {scratch} B of scratch, {spills} spilled VGPRs"
                assert vgprs <= 128, f"{name}: {vgprs} VGPRs"
    assert seen == {"k_loop_filter_simpleENS", "k_loop_filter_simple_bENS"}, seen


def skip_inner_of(coeffs, parts):
    """prepare_filter_mask: the inner edges are skipped for a macroblock with no non-zero coefficient that is not split"""
    c = np.abs(coeffs.astype(np.int32))
    split = parts != 0
    nz = c[:, :16, 1:].sum((1, 2)) + np.where(split, c[:, :16, 0].sum(1), 0) + c[:, 16:24].sum((1, 2)) + \
        np.where(split, 0, c[:, 24].sum(1))
    return ~(split | (nz > 0))


def restate(y, sd, seg, skip_inner, mbw, mbh):
    """the simple filter over a luma plane with the limits of the segment data (what the device reads)"""
    sd = np.asarray(sd).reshape(4, 11)
    seg = np.asarray(seg)
    out = y.copy()
    simple_filter_plane(out, mbw, mbh, sd[seg, 6], sd[seg, 7], sd[seg, 8], skip_inner)
    return out


needs_libwebp = pytest.mark.skipif(webp_decode.libwebp() is None, reason="no libwebp in this image")


@needs_libwebp
@pytest.mark.parametrize("W,H,seed", [(176, 144, 3), (320, 192, 5), (640, 352, 7)])
def test_restatement_matches_libwebp_on_key_frames(W, H, seed):
    """the oracle's key frame with filter_type = 1 in its first partition (the reference's own encode_header): libwebp decodes
    it to the restatement applied to the oracle's pre-filter reconstruction; chroma is not filtered"""
    from bitstream_cases import ref_encode_header, ref_header_lib
    from entropy_cases import nz_counts
    from oracle_lib import Oracle
    from vp8oclenc_amd import bitstream
    from vp8oclenc_amd.driver import InterPathDriver
    if ref_header_lib() is None:
        pytest.skip("oracle/_ref is not built")
    s = SynthSequence(W, H, seed=seed)
    ora = Oracle(s.W, s.H, -1.0)
    do = InterPathDriver(ora, s.W, s.H, gop_size=150)
    assert do.encode_frame(*s.frame(0)) is None
    res = do.last_key
    coeffs, parts = np.ascontiguousarray(res["MB_coeffs"]), np.ascontiguousarray(res["MB_parts"])
    nz = nz_counts(coeffs, parts)
    mbw, mbh = s.W // 16, s.H // 16
    mbs = mbw * mbh
    st = Oracle.stages()
    probs, denom = np.zeros(1056, np.uint32), np.zeros(1056, np.uint32)
    ctx3 = np.zeros(mbs * 25, np.uint8)
    st.count_probs(coeffs, nz, parts, probs, denom, ctx3, mbh, mbw, 1)
    st.num_div_denom(probs, denom, 1)
    p0 = bitstream.default_probs(probs, denom)
    step = mbs * 3200 + 4096
    out, sizes = np.zeros(step, np.uint8), np.zeros(1, np.int32)
    st.encode_coefficients(coeffs, nz, parts, out, sizes, ctx3, p0, mbh, mbw, 1, step)
    sd = np.asarray(res["segments"]).reshape(4, 11)
    hdr = ref_encode_header(s.W, s.H, (1, 1, 1), sd, res["MB_segment_id"], nz, p0, denom, api.skip_prob(nz), modes=res.get("modes"),
                            loop_filter_type=1, sharpness=int(res["sharpness"]))
    frame = bitstream.gather_frame(hdr, [out[:sizes[0]]]).tobytes()
    Y, U, V = webp_decode.decode_key_frame(frame)
    want = restate(res["prefilter_Y"], sd, res["MB_segment_id"], skip_inner_of(coeffs, parts), mbw, mbh)
    assert (want != res["prefilter_Y"]).any(), "the filter did nothing: the comparison would show nothing"
    assert np.array_equal(Y, want)
    assert np.array_equal(U, res["prefilter_U"]) and np.array_equal(V, res["prefilter_V"])
    ora.close()
