#!/usr/bin/env python3
"""What cyclic intra refresh costs and what it repairs (profiles/README.md, "Intra refresh"), from two conformant IVF files of the same
synthetic sequence -- one coded without refresh, one with period P -- as scripts/encode_ivf.py writes them:
    python scripts/encode_ivf.py off.ivf --width W --height H --frames N --gop G --conformant [--intra-refresh P] ...
Needs no GPU: the files are decoded by the RFC 6386 decoder of tests/vp8_decode.py.  Printed as one JSON line: bytes and overall luma
PSNR against the source of both files, and the recovery of the refreshed one -- the decoder's three reference buffers are replaced by
grey after frame K (a receiver that lost everything), and the luma PSNR of the damaged decoding against the intact one is taken one and
two periods later, next to the same figures for the file without refresh.  Convergence is reported, not promised: motion vectors are not
constrained to the refreshed area, and GOLDEN / ALTREF can carry damage back in.
    python scripts/refresh_recovery.py off.ivf on.ivf --period P --lose-after K [--seed 1]"""
import argparse, json, os, struct, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def ivf_frames(path):
    data = open(path, "rb").read()
    assert data[:4] == b"DKIF", path
    w, h = struct.unpack_from("<HH", data, 12)
    pos, out = struct.unpack_from("<H", data, 6)[0], []
    while pos + 12 <= len(data):
        n = struct.unpack_from("<I", data, pos)[0]
        out.append(data[pos + 12:pos + 12 + n])
        pos += 12 + n
    return w, h, out


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 99.0 if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def decode(frames, lose_after=None):
    """-> the luma of every decoded frame; lose_after = K: behind frame K the decoder's references become grey"""
    import vp8_decode
    dec, out = vp8_decode.Decoder(), []
    for t, b in enumerate(frames):
        _, planes = dec.decode(b)
        out.append(planes[0].copy())
        if lose_after is not None and t == lose_after:
            grey = tuple(np.full_like(p, 128) for p in planes)
            for k in dec.ref:
                dec.ref[k] = grey
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("off"); ap.add_argument("on")
    ap.add_argument("--period", type=int, required=True)
    ap.add_argument("--lose-after", type=int, required=True, metavar="K")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    from vp8oclenc_amd.synth import SynthSequence
    res = dict(what="intra refresh: cost and recovery", period=a.period, lose_after=a.lose_after)
    for name, path in (("off", a.off), ("on", a.on)):
        w, h, frames = ivf_frames(path)
        if not 0 <= a.lose_after < len(frames) - 1:
            sys.exit(f"--lose-after {a.lose_after}: {path} holds {len(frames)} frames, and a frame behind the loss is needed")
        seq = SynthSequence(w, h, seed=a.seed)
        intact = decode(frames)
        src = [seq.frame(t)[0][:h, :w] for t in range(len(frames))]
        damaged = decode(frames, a.lose_after)
        at = {f"after_{k}_periods": a.lose_after + k * a.period for k in (1, 2) if a.lose_after + k * a.period < len(frames)}
        res[name] = dict(size=[w, h], frames=len(frames), bytes=sum(len(f) for f in frames),
                         psnr_y_overall=round(psnr(np.stack(intact), np.stack(src)), 3),
                         damaged_vs_intact_psnr_y={k: round(psnr(damaged[t], intact[t]), 2) for k, t in at.items()},
                         damaged_vs_intact_psnr_y_next_frame=round(psnr(damaged[a.lose_after + 1], intact[a.lose_after + 1]), 2))
    res["bytes_ratio"] = round(res["on"]["bytes"] / res["off"]["bytes"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
