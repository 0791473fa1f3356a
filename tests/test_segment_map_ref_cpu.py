"""tests/segment_map_ref.py, the expected result of a frame coded under a segment map assembled from the oracle's stages, held to what
it must reduce to: with the constant map 3 it is the default's frame (tests/pipeline.py at ssim_target = -1), and a macroblock's results
depend on its own byte of the map alone."""
import os

import numpy as np

from pipeline import load_meta, run_inter_frame
from segment_map_ref import run_mapped_inter_frame

KEYS = ["MB_parts", "MB_reference_frame", "MB_vectors", "MB_coeffs", "MB_segment_id", "MB_non_zero_coeffs", "mb_mask",
        "prefilter_Y", "prefilter_U", "prefilter_V", "recon_Y", "recon_U", "recon_V"]


def test_assembly_reduces_to_the_default_and_is_local_to_the_macroblock(oracle_stages):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g96x64_3refs.npz"))
    meta = load_meta(z)
    cur = tuple(np.ascontiguousarray(z[f"in_cur_{p}"]) for p in "YUV")
    refs = [tuple(np.ascontiguousarray(z[f"in_ref{r}_{p}"]) for p in "YUV") for r in range(3)]
    sd, flags = z["segments"], (meta["use_golden"], meta["use_altref"])
    mbs = (meta["W"] // 16) * (meta["H"] // 16)
    default = run_inter_frame(oracle_stages, cur, refs, sd, *flags, -1.0)
    same = run_mapped_inter_frame(oracle_stages, cur, refs, sd, *flags, np.full(mbs, 3))
    for k in KEYS:
        assert np.array_equal(default[k], same[k]), k
    assert np.array_equal(default["MB_SSIM"].view(np.uint32), same["MB_SSIM"].view(np.uint32))
    seg_map = np.random.default_rng(1).integers(0, 4, mbs)
    mixed = run_mapped_inter_frame(oracle_stages, cur, refs, sd, *flags, seg_map)
    const = [run_mapped_inter_frame(oracle_stages, cur, refs, sd, *flags, np.full(mbs, s)) for s in range(4)]
    assert not np.array_equal(const[0]["MB_coeffs"], const[3]["MB_coeffs"])
    for mb in range(mbs):
        c = const[seg_map[mb]]
        assert np.array_equal(mixed["MB_coeffs"][mb], c["MB_coeffs"][mb]) and mixed["MB_non_zero_coeffs"][mb] == c["MB_non_zero_coeffs"][mb]
        assert mixed["MB_SSIM"][mb].view(np.uint32) == c["MB_SSIM"][mb].view(np.uint32)
    assert np.array_equal(mixed["MB_segment_id"], seg_map)
