"""--dump-outputs DIR: what the timed path left behind after its last step, as .npy files that two builds can be held against each other
with.  Per GOP chunk: the filtered reconstruction (the frame the next one is searched against) and the macroblock results of the last frame
(vp8hip_download_results: vectors, reference, partitions, segment, SSIM, coefficients).  Every array whole as CRC-32s (float64, exact), and a
fixed, seeded sample of the values themselves (float32): at most 48 chunks, a fixed number of pixels and macroblocks each, so that the files
stay below 64 MB at every geometry and chunk count."""
from __future__ import annotations

import os
import zlib

MAX_BYTES = 64 << 20
SEED = 20261015
MAX_CHUNKS = 48          # chunks whose values are sampled (the CRCs cover every chunk)
PIXELS_Y, PIXELS_UV = 65536, 16384
MBS, MBS_COEFFS = 1024, 256

MB_KEYS = ("MB_vectors", "MB_reference_frame", "MB_parts", "MB_segment_id", "MB_SSIM", "MB_coeffs")


def dump_outputs(leg, path):
    """writes DIR/<name>.npy for the chunks of `leg` as they stand (every driver resolved); returns the names written"""
    import numpy as np
    rng = np.random.default_rng(SEED)
    G, W, H, n = leg.G, leg.W, leg.H, leg.mbs
    sampled = sorted(rng.choice(G, MAX_CHUNKS, replace=False).tolist()) if G > MAX_CHUNKS else list(range(G))
    pos = [np.sort(rng.choice(W * H, min(PIXELS_Y, W * H), replace=False))] + \
          [np.sort(rng.choice(W * H // 4, min(PIXELS_UV, W * H // 4), replace=False)) for _ in range(2)]
    mb = np.sort(rng.choice(n, min(MBS, n), replace=False))
    mb_c = np.sort(rng.choice(n, min(MBS_COEFFS, n), replace=False))
    out = {"chunk_index": np.array(sampled, np.float64),
           "recon_crc32": np.zeros((G, 3), np.float64), "mb_crc32": np.zeros((G, len(MB_KEYS)), np.float64),
           "recon_y": [], "recon_u": [], "recon_v": [],
           "mb_vectors": [], "mb_reference_frame": [], "mb_parts": [], "mb_segment_id": [], "mb_ssim": [], "mb_coeffs": []}
    for k, d in enumerate(leg.drv):
        d.resolve()
        planes = d.hip.download_last()
        res = d.hip.download_results(recon=False)
        out["recon_crc32"][k] = [zlib.crc32(p.tobytes()) for p in planes]
        out["mb_crc32"][k] = [zlib.crc32(np.ascontiguousarray(res[key]).tobytes()) for key in MB_KEYS]
        if k not in sampled:
            continue
        for name, p, q in zip(("recon_y", "recon_u", "recon_v"), planes, pos):
            out[name].append(p.reshape(-1)[q])
        out["mb_vectors"].append(res["MB_vectors"][mb])
        out["mb_reference_frame"].append(res["MB_reference_frame"][mb])
        out["mb_parts"].append(res["MB_parts"][mb])
        out["mb_segment_id"].append(res["MB_segment_id"][mb])
        out["mb_ssim"].append(res["MB_SSIM"][mb])
        out["mb_coeffs"].append(res["MB_coeffs"][mb_c])
    arrays = {}
    for name, v in out.items():
        a = np.stack(v) if isinstance(v, list) else v
        arrays[name] = a if a.dtype == np.float64 else a.astype(np.float32)
    total = sum(a.nbytes for a in arrays.values())
    if total > MAX_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes, more than {MAX_BYTES}")
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(arrays)
