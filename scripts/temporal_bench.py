#!/usr/bin/env python3
"""What temporal layers cost in bytes and quality at a fixed quantiser pair (profiles/README.md, "Temporal layers"): the sequences of
scripts/arf_bench.py --effect (a clean synthetic sequence and the same under Gaussian noise), one GOP, scheduled alt-refs off in every
run, coded with 1, 2 and 3 layers.  One JSON line per run: the bytes of the stream and of the sub-streams a forwarding unit makes of it
(temporal_id <= 0, <= 1), vpxenc's overall PSNR and SSIM over all frames measured on the device against the source, the frames per
layer and how many were not loop-filtered.  Speed is scripts/frame_bench.py --temporal-layers N.
    python scripts/temporal_bench.py [--size 640x352] [--frames 48] [--gop 48] [--qi 20:60]"""
import argparse
import json
import os
import sys

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="640x352")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--gop", type=int, default=48)
    ap.add_argument("--qi", default="20:60")
    a = ap.parse_args()
    from vp8oclenc_amd import api
    from vp8oclenc_amd.synth import SynthSequence
    w, h = (int(x) for x in a.size.split("x"))
    qi = tuple(int(x) for x in a.qi.split(":"))
    seq = SynthSequence(w, h, seed=7)
    rng = np.random.default_rng(1)
    clean = [seq.frame(t) for t in range(a.frames)]
    noisy = [tuple(np.clip(p.astype(np.int64) + np.rint(rng.normal(0, 4, p.shape)).astype(np.int64), 0, 255).astype(np.uint8) for p in f) for f in clean]
    for name, frames in (("clean", clean), ("noisy", noisy)):
        for layers in (1, 2, 3):
            drv = api.NativeDriver(seq.W, seq.H, gop_size=a.gop, altref_range=a.gop + 1, qi_min=qi[0], qi_max=qi[1], quality_stats=1, num_partitions=4)
            drv.set_temporal_layers(layers)
            by_layer, count, golden, inter_mbs = [0, 0, 0], [0, 0, 0], 0, 0
            for f in frames:
                key = drv.encode_frame_host(*f)
                size = len(drv.get_frame())
                key = drv.resolve() or key
                info = drv.frame_layer()
                by_layer[info.temporal_id] += size
                count[info.temporal_id] += 1
                if not key:
                    r = drv.hip.download_results(recon=False)["MB_reference_frame"]
                    golden += int((r == 1).sum())
                    inter_mbs += r.size
            q = drv.quality_summary()
            print(json.dumps(dict(what="temporal layers", sequence=name, size=[seq.W, seq.H], frames=a.frames, gop=a.gop, qi=list(qi), layers=layers, bytes=sum(by_layer),
                                  bytes_tid0=by_layer[0], bytes_tid01=by_layer[0] + by_layer[1], frames_per_layer=count, psnr_overall=round(q.psnr_all, 3),
                                  ssim_overall=round(q.ssim_all, 5), golden_share=round(golden / max(inter_mbs, 1), 4))), flush=True)
            drv.close()


if __name__ == "__main__":
    main()
