#!/usr/bin/env python3
"""Hidden alternate reference frames measured (profiles/README.md, "Hidden alt-ref"): nothing here is a threshold.

  --kernel   k_arf_filter_b by the launch's own events (vp8hip_profile_enable on the input side's stage: the filter launch and the pack
             launch behind it, minus the pack launch alone) at 1920x1080 and 3840x2160 for windows of 3 and 7, beside a device-to-device
             hipMemcpyAsync of the window's bytes between two events (the memory floor; best and mean) and beside one coded frame of the
             same process's driver loop BY THE HOST'S CLOCK (frames per second of the native video loop, no frames out).
  --effect   one clean and one noisy synthetic sequence at a fixed quantiser pair with and without --arf PERIOD[:FRAMES[:STRENGTH]]
             (the placement of tests/arf_ref.schedule, scheduled shown alt-refs off in both runs): total bytes with the hidden frames,
             overall PSNR and SSIM of the shown frames, the share of inter macroblocks that chose ALTREF.
One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def d2d_copy_ms(nbytes, reps):
    """hipMemcpyAsync device to device of nbytes distinct bytes between two events on the null stream -> (best, mean) in ms.  The calls
    go to the HIP runtime the library itself is linked with (the one already in this process), through ctypes."""
    import ctypes as C
    from vp8oclenc_amd import api
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    src, dst = api.to_device(np.tile(np.arange(256, dtype=np.uint8), nbytes // 256 + 1)[:nbytes]), api.DeviceBuffer(nbytes)
    e0, e1, ms, got = C.c_void_p(), C.c_void_p(), C.c_float(), []
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    for _ in range(reps + 2):
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None) == 0      # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        got.append(float(ms.value))
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    src.free()
    dst.free()
    got = got[2:]
    return min(got), sum(got) / len(got)


def kernel_times(reps):
    from vp8oclenc_amd import api
    from vp8oclenc_amd.synth import bench_frames
    for W0, H0 in ((1920, 1080), (3840, 2160)):
        W, H, source, _ = bench_frames(W0, H0, 1, 8)
        dev = [tuple(api.to_device(p) for p in f) for f in source]
        ptrs = [tuple(p.data_ptr() for p in f) for f in dev]
        hip = api.Vp8Hip(W, H)
        if (W0, H0) != (W, H):
            hip.set_source_size(W0, H0)
        hip.profile_enable(["pack"])
        hip.set_current_device(*ptrs[0])
        hip.arf_filter_device(ptrs[:3], 1, 3)      # (first use: the staging buffer)
        hip.profile_read()
        for _ in range(reps):
            hip.set_current_device(*ptrs[0])
        pack_ms = hip.profile_read()["pack"][0] / reps
        out = dict(what="k_arf_filter_b", size=[W0, H0], pack_launch_ms=round(pack_ms, 4))
        for n in (3, 7):
            for _ in range(reps):
                hip.arf_filter_device(ptrs[:n], n // 2, 3)
            ms, launches = hip.profile_read()["pack"]
            assert launches == 2 * reps
            out[f"window_{n}_ms"] = round(ms / reps - pack_ms, 4)
            best, mean = d2d_copy_ms(n * (W0 * H0 * 3 // 2), reps)
            out[f"window_{n}_d2d_copy_ms_best_mean"] = [round(best, 4), round(mean, 4)]
            out[f"window_{n}_weights"] = hip.arf_result()
        hip.close()
        drv = api.NativeDriver(W, H, gop_size=150, device_params=1, check_ssim=1, **(dict(src_width=W0, src_height=H0) if (W0, H0) != (W, H) else {}))
        drv.encode_video_device_no_frames(8, ptrs)
        drv.hip.synchronize()
        t0 = time.perf_counter()
        drv.encode_video_device_no_frames(40, ptrs)
        drv.hip.synchronize()
        out["one_coded_frame_wall_ms"] = round((time.perf_counter() - t0) / 40 * 1e3, 4)
        drv.close()
        print(json.dumps(out), flush=True)


def effect(arf, W, H, frames_total, gop, qi):
    import arf_ref as ref
    from vp8oclenc_amd import api
    from vp8oclenc_amd.synth import SynthSequence
    period, nmax, strength = list(arf) + [7, 3][len(arf) - 1:]
    seq = SynthSequence(W, H, seed=7)
    rng = np.random.default_rng(1)
    clean = [seq.frame(t) for t in range(frames_total)]
    noisy = [tuple(np.clip(p.astype(np.int64) + np.rint(rng.normal(0, 4, p.shape)).astype(np.int64), 0, 255).astype(np.uint8) for p in f) for f in clean]
    for name, frames in (("clean", clean), ("noisy", noisy)):
        for on in (False, True):
            drv = api.NativeDriver(seq.W, seq.H, gop_size=gop, altref_range=gop + 1, qi_min=qi[0], qi_max=qi[1], quality_stats=1, num_partitions=4)
            placement = ref.schedule(frames_total, gop, period, nmax) if on else {}
            if on:
                drv.set_arf(strength + 1)
            total = hidden = altref = inter_mbs = 0
            for ev in ref.events(frames_total, placement):
                if ev[0] == "hidden":
                    _, _, lo, n, centre = ev
                    drv.encode_arf_host(frames[lo:lo + n], centre)
                    total += len(drv.get_frame())
                    hidden += 1
                    continue
                key = drv.encode_frame_host(*frames[ev[1]])
                total += len(drv.get_frame())
                key = drv.resolve() or key
                if not key:
                    r = drv.hip.download_results(recon=False)["MB_reference_frame"]
                    altref += int((r == 2).sum())
                    inter_mbs += r.size
            q = drv.quality_summary()
            print(json.dumps(dict(what="effect", sequence=name, size=[seq.W, seq.H], frames=frames_total, gop=gop, qi=list(qi), arf=[period, nmax, strength] if on else None,
                                  hidden_frames=hidden, bytes=total, psnr_overall=round(q.psnr_all, 3), ssim_overall=round(q.ssim_all, 5), shown_frames=int(q.frames),
                                  altref_share=round(altref / max(inter_mbs, 1), 4))), flush=True)
            drv.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--effect", action="store_true")
    ap.add_argument("--arf", default="8", help="PERIOD[:FRAMES[:STRENGTH]] (default frames 7, strength 3)")
    ap.add_argument("--size", default="640x352")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--gop", type=int, default=48)
    ap.add_argument("--qi", default="20:60")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.kernel:
        kernel_times(a.reps)
    if a.effect:
        w, h = (int(x) for x in a.size.split("x"))
        effect([int(x) for x in a.arf.split(":")], w, h, a.frames, a.gop, tuple(int(x) for x in a.qi.split(":")))


if __name__ == "__main__":
    main()
