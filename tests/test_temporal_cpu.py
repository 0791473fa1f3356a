"""Temporal layers without a GPU: vp8host_temporal_step against the Python restatement of include/vp8hip_host.h's rule
(tests/temporal_ref.py); the closure property a forwarding unit relies on, simulated on frame numbers; the host first-partition coder
with the two header values of a layered frame, read back by tests/vp8_parse.py; a layered sequence from the CPU oracle's frame loop
through the RFC 6386 decoder of tests/vp8_decode.py, whole and with the upper layers dropped; and the rule and the coder under the
address and undefined-behaviour sanitizers in a stand-alone program.  Everything is exact: no tolerances.  tests/test_gpu_temporal.py
holds the native driver to the same restatement and the same loop."""
import glob
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as ref
from vp8oclenc_amd import api, bitstream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "bitstream", "inter_*.npz")))
SAN = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include")]


# ---- 1. the host function against the restatement -----------------------------------------------------------------------------------------
def test_the_host_rule_equals_the_restatement():
    for layers in (1, 2, 3):
        for p in range(41):
            for mask in range(4):
                assert api.temporal_step(layers, p, mask) == ref.step(layers, p, mask), (layers, p, mask)
    for layers, p in ((0, 0), (4, 0), (-1, 2), (2, -1), (3, -7)):
        assert ref.step(layers, p) is None
        with pytest.raises(ValueError):
            api.temporal_step(layers, p)
    assert (api.REFRESH_LAST, api.REFRESH_GOLDEN, api.REFRESH_NONE, api.REFRESH_ALL) == (ref.LAST, ref.GOLDEN, ref.NONE, ref.ALL)
    # layers = 1 is "off": every frame in layer 0, LAST / LAST
    assert all(ref.step(1, p, 3) == dict(temporal_id=0, use_golden=0, refresh=ref.LAST, layer_sync=0) for p in range(1, 41))


# ---- 2. the closure property ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_mask", [3, 0])
@pytest.mark.parametrize("layers", [2, 3])
def test_dropping_the_upper_layers_changes_no_buffer_a_kept_frame_reads(layers, ref_mask):
    """64 frames with key frames at irregular places (so the pattern restarts at every residue of p): three buffers that hold frame
    numbers follow the refresh rule.  For K = 0, 1: in the stream of the frames with temporal_id <= K every buffer a kept frame searches
    holds the frame it holds in the full stream, and never a frame of a higher layer than K -- nor of a higher layer than the frame's."""
    keys = {0, 5, 6, 19, 30, 33, 47}
    recs = ref.records(layers, keys, 64, ref_mask)
    assert [r["p"] for r in recs[:8]] == [0, 1, 2, 3, 4, 0, 0, 1]
    assert {r["temporal_id"] for r in recs} == set(range(layers))
    full = ref.simulate(recs, 2)
    assert len(full) == 64
    for K in (0, 1):
        kept = ref.simulate(recs, K)
        assert sorted(kept) == [t for t, r in enumerate(recs) if r["temporal_id"] <= K]
        for t, bufs in kept.items():
            assert bufs == full[t], (K, t)
            for b, (number, tid) in bufs.items():
                assert tid <= min(K, recs[t]["temporal_id"]) and number < t, (K, t, b)
            assert recs[t]["layer_sync"] == int(all(tid == 0 for _, tid in bufs.values()) and recs[t]["temporal_id"] > 0), (K, t)
    if layers == 3 and ref_mask & 1:      # GOLDEN, where it is searched, is the frame in front: newer than LAST
        assert any(r["use_golden"] for r in recs)
        for t, r in enumerate(recs):
            if r["use_golden"]:
                assert full[t][ref.GOLDEN][0] == t - 1 and full[t][ref.LAST][0] == t - 3
    # tl0_pic_idx: a running index of the layer-0 frames
    assert [r["tl0_pic_idx"] for r in recs if r["temporal_id"] == 0] == list(range(sum(r["temporal_id"] == 0 for r in recs)))


# ---- 3. the two header values in the host bitstream -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_a_layered_frame_parses_as_one_and_an_ordinary_frame_keeps_its_bytes(path):
    import vp8_parse as vp
    z = np.load(path)
    opt = lambda k: np.ascontiguousarray(z[k]) if k in z.files else None
    W, H = int(z["W"]), int(z["H"])

    def header(flags):
        return bitstream.encode_header(W, H, flags, z["sd"], z["seg"], z["nz"], z["probs"], z["denom"], int(z["skip_prob"]), ref_frame=opt("ref_frame"),
                                       parts=opt("parts"), vectors=opt("vectors"), is_inter=opt("is_inter"), modes=opt("modes"),
                                       replaced=int(z["replaced"]), sharpness=int(z["sharpness"]), partitions_log2=int(z["partitions_log2"]))[0]

    assert np.array_equal(header(tuple(int(x) for x in z["flags"])), z["header"])      # the reference's bytes, as before
    P = 1 << int(z["partitions_log2"])
    tokens = [np.zeros(4096, np.uint8)] * P      # (no coefficient partitions in the fixture: zeros decode to some tokens, the same for all)
    frames = {}
    for name, fl in (("last", (0, 0, 0)), ("golden", (0, api.GOLDEN_ONLY, 0)), ("none", (0, api.REFRESH_NOTHING, 0)), ("none, is_altref set", (0, api.REFRESH_NOTHING, 1))):
        st = vp.StreamState()
        st.width, st.height = W, H      # (what a key frame would have set)
        frames[name] = vp.parse_frame(bitstream.gather_frame(header(fl), tokens).tobytes(), st)
    want = {"last": (1, 0, 0, 0, 0, 1), "golden": (1, 1, 0, 0, 0, 0), "none": (1, 0, 0, 0, 0, 0), "none, is_altref set": (1, 0, 0, 0, 0, 0)}
    for name, f in frames.items():
        got = (f.show, f.refresh_golden, f.refresh_altref, f.copy_to_golden, f.copy_to_altref, f.refresh_last)
        assert not f.key and got == want[name] and f.refresh_entropy == 0, (name, got)
        for k in ("ref_frame", "mv_mode", "mvs", "is_inter", "segment_id", "skip"):      # the rest of the frame is unchanged
            assert np.array_equal(getattr(f, k), getattr(frames["last"], k)), (name, k)


# ---- 4. a layered sequence through the decoder, whole and thinned ----------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [2, 3])
def test_an_oracle_sequence_decodes_with_its_upper_layers_dropped(layers):
    import arf_ref
    import vp8_decode
    w, h, total = 64, 48, 13
    frames = arf_ref.noisy_pan(w, h, total, seed=w + total)
    recs = ref.oracle_loop(frames, layers, conformant=True, gop_size=9, altref_range=10, qi_min=10, qi_max=60)
    assert [r["key"] for r in recs] == [t in (0, 9) for t in range(total)]
    assert [r["layer"] for r in recs] == [{k: r[k] for k in ("temporal_id", "use_golden", "refresh", "layer_sync", "tl0_pic_idx")}
                                          for r in ref.records(layers, {9}, total)]
    stream = [ref.record_bytes(r, w, h, 2) for r in recs]
    golden_mbs = 0
    for keep in (2, 1, 0):
        dec = vp8_decode.Decoder()
        for r, b in zip(recs, stream):
            if r["layer"]["temporal_id"] > keep:
                continue
            before = dict(dec.ref) if getattr(dec, "ref", None) else {}
            f, planes = dec.decode(b)
            for name, g, want in zip("YUV", planes, r["recon"]):
                assert np.array_equal(g, want), (keep, r["t"], name)
            if r["layer"]["refresh"] == ref.GOLDEN:
                assert dec.ref[1] is before[1] and dec.ref[2] is planes and dec.ref[3] is before[3]
            elif r["layer"]["refresh"] == ref.NONE:
                assert all(dec.ref[k] is before[k] for k in (1, 2, 3))
            if keep == 2 and r["layer"]["use_golden"]:
                golden_mbs += int((f.ref_frame[f.is_inter.astype(bool)] == 2).sum())
    if layers == 3:
        assert golden_mbs > 0      # the top layer uses the middle one


# ---- 5. the sanitizers ----------------------------------------------------------------------------------------------------------------------
def test_the_rule_and_the_header_coder_are_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "temporal_sanitize")
    csrc = os.path.join(ROOT, "vp8oclenc_amd", "csrc")
    subprocess.run(SAN + [os.path.join(ROOT, "scripts", "native", "temporal_sanitize.cpp"), os.path.join(csrc, "vp8_host.cpp"), os.path.join(csrc, "vp8_bitstream.cpp"),
                          "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("clean"), r.stdout + r.stderr


def test_the_library_exports_the_entry_points():
    lib = api.load_library()
    for name in ("vp8host_temporal_step", "vp8hip_loop_filter_refresh", "vp8drv_set_temporal_layers", "vp8drv_get_frame_layer"):
        assert hasattr(lib, name), name
