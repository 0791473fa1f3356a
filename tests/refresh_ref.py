"""Cyclic intra refresh restated in Python from the TEXT of include/vp8hip_host.h (not from vp8host_intra_refresh_forced's C++): the
rule, the expected result of a refresh frame assembled from the oracle's EXISTING stages (one vp8o_check_ssim call per segment on a
doctored SSIM array: no new oracle code), and the CPU oracle's frame loop with the rule -- the expected bytes and reconstructions
tests/test_gpu_refresh.py holds the context and the native driver to.  tests/test_refresh_cpu.py holds the host functions and the
host header coder to the rule without a GPU.  Test infrastructure."""
import numpy as np

import temporal_ref

PERIOD_MIN, PERIOD_MAX = 4, 1024


def forced(period, q, r, c):
    """macroblock (row r, column c) is forced at phase q iff (c + 2 r) mod P == q mod P"""
    assert PERIOD_MIN <= period <= PERIOD_MAX and q >= 0
    return (c + 2 * r) % period == q % period


def forced_map(mbw, mbh, period, q):
    """-> bool [mbh][mbw]"""
    r, c = np.mgrid[0:mbh, 0:mbw]
    return (c + 2 * r) % period == q % period


def refresh_frame(cur, sd, inter, period, q):
    """The expected result of a refresh: inter = the inter frame's outputs (prefilter_Y/U/V, MB_coeffs, MB_parts, MB_segment_id, MB_SSIM)
    -> a dict with the same keys updated + modes, is_inter, forced (the count), MB_non_zero_coeffs, mb_mask.
    One vp8o_check_ssim call per distinct segment s among the forced macroblocks: SSIM doctored to -2 at the forced macroblocks of
    segment s and +2 elsewhere, target -1.5 (SSIM lies in [-1, 1]: exactly one attempt is made, the AQ row's, and kept), segment data
    whose AQ row (2) is a copy of row s.  No forced macroblock is another's neighbour, so the order of the calls does not matter."""
    from oracle_lib import Oracle, oracle_intra
    y = np.ascontiguousarray(cur[0])
    H, W = y.shape
    mbw, mbh = W // 16, H // 16
    mbs = mbw * mbh
    fm = forced_map(mbw, mbh, period, q).reshape(-1)
    seg0 = np.asarray(inter["MB_segment_id"]).reshape(-1).copy()
    state = {"recon_Y": inter["prefilter_Y"], "recon_U": inter["prefilter_U"], "recon_V": inter["prefilter_V"], "MB_coeffs": inter["MB_coeffs"],
             "MB_parts": inter["MB_parts"], "MB_segment_id": seg0, "MB_SSIM": inter["MB_SSIM"]}
    state = {k: np.ascontiguousarray(v).copy() for k, v in state.items()}
    ssim0 = state["MB_SSIM"].copy()
    sd = np.ascontiguousarray(sd, np.int32).reshape(4, 11)
    modes = np.zeros((mbs, 16), np.int32)
    is_inter = np.ones(mbs, np.int32)
    new_ssim = ssim0.copy()
    for s in sorted(set(int(v) for v in seg0[fm])):
        pick = fm & (seg0 == s)
        sd_s = sd.copy()
        sd_s[2] = sd[s]
        doctored = np.full(mbs, 2.0, np.float32)
        doctored[pick] = -2.0
        state["MB_SSIM"] = doctored
        r = oracle_intra().check_ssim(cur, sd_s, -1.5, state)
        assert r["replaced"] == int(pick.sum()) and np.array_equal(r["is_inter"] == 0, pick)
        assert (r["MB_segment_id"][pick] == 2).all() and (r["MB_SSIM"][pick] >= -1.0).all()
        modes[pick] = r["modes"][pick]
        is_inter[pick] = 0
        new_ssim[pick] = r["MB_SSIM"][pick]
        for k in ("recon_Y", "recon_U", "recon_V", "MB_coeffs", "MB_parts"):
            state[k] = r[k]
        state["MB_segment_id"] = seg0.copy()      # the segment id does not change
    state["MB_SSIM"] = new_ssim
    assert (state["MB_parts"][fm] == 2).all()
    nz, mask = np.zeros(mbs, np.int32), np.zeros(mbs, np.int32)
    Oracle.stages().prepare_filter_mask(np.ascontiguousarray(state["MB_coeffs"]), nz, np.ascontiguousarray(state["MB_parts"]), mask, W, H)
    assert (mask[fm] == -1).all()
    return dict(prefilter_Y=state["recon_Y"], prefilter_U=state["recon_U"], prefilter_V=state["recon_V"], MB_coeffs=state["MB_coeffs"],
                MB_parts=state["MB_parts"], MB_segment_id=seg0, MB_SSIM=new_ssim, modes=modes, is_inter=is_inter, forced=int(fm.sum()),
                MB_non_zero_coeffs=nz, mb_mask=mask)


# ---- the CPU oracle's frame loop with the rule ------------------------------------------------------------------------------------------
def refresh_driver(backend, w, h, layers, schedule, **cfg):
    """tests/temporal_ref.layered_driver with frame_body's refresh: behind the transform of a frame whose ending is LAST, at the period
    schedule(t) names for stream frame t (0 = off), phase q = the LAST-refreshing inter frames since the last key frame"""
    if layers > 1:
        base = temporal_ref.layered_driver(backend, w, h, layers, **cfg)
    else:      # the reference's own loop (references and ladder from the GOP state), with the layered driver's two counters
        from vp8oclenc_amd.driver import InterPathDriver

        class PlainDriver(InterPathDriver):
            p = 0
            layer = None

            def _key_frame(self, y, u, v):
                self.p = 1
                self.layer = temporal_ref.step(1, 0, self.ref_mask)
                return super()._key_frame(y, u, v)

            def encode_frame(self, y, u, v, force_key=False):
                out = super().encode_frame(y, u, v, force_key)
                if out is not None:
                    self.layer = temporal_ref.step(1, self.p, self.ref_mask)
                    self.p += 1
                return out

        base = PlainDriver(backend, w, h, **cfg)

    class RefreshDriver(type(base)):
        q = 0
        t = -1
        info = None

        def _key_frame(self, y, u, v):
            self.q = 0
            self.info = dict(q=0, forced=0, period=self.period_now)
            return super()._key_frame(y, u, v)

        def encode_frame(self, y, u, v, force_key=False):
            self.t += 1
            self.period_now = P = schedule(self.t)
            be = self.be
            real_transform, me = be.inter_transform, self
            rule = {}

            def transform_and_refresh(pg, pa, ug, ua):
                real_transform(pg, pa, ug, ua)
                if rule:      # (the oracle backend's GOLDEN ending transforms once more, to rotate its buffers: not the frame's transform)
                    return
                t = temporal_ref.step(layers, me.p, me.ref_mask)
                rule.update(t)
                me.info = dict(q=me.q, forced=0, period=P)
                be._refresh = None
                if P and t["refresh"] == temporal_ref.LAST:
                    fm = forced_map(w // 16, h // 16, P, me.q)
                    if fm.any():
                        o = be._out
                        r = refresh_frame(be._cur, be._sd, o, P, me.q)
                        for k in ("MB_coeffs", "MB_parts", "MB_SSIM", "prefilter_Y", "prefilter_U", "prefilter_V"):
                            o[k][...] = r[k]
                        be.upload_recon(r["prefilter_Y"], r["prefilter_U"], r["prefilter_V"])
                        be.upload_mb_data(r["MB_coeffs"], r["MB_parts"], r["MB_segment_id"])
                        be._refresh = r
                        me.info["forced"] = r["forced"]

            be.inter_transform = transform_and_refresh
            try:
                out = super().encode_frame(y, u, v, force_key)
            finally:
                be.inter_transform = real_transform
            if out is not None:
                if rule["refresh"] == temporal_ref.LAST:
                    self.q += 1
                r = be._refresh
                if r is not None:      # the header takes the intra information: the rule's macroblocks, replaced = their number
                    out["modes"], out["is_inter"], out["replaced"] = r["modes"], r["is_inter"], r["forced"]
            return out

    base.__class__ = RefreshDriver
    return base


def oracle_loop(frames, layers, schedule, conformant=False, force_key=(), **cfg):
    """tests/temporal_ref.oracle_loop with the refresh -> records dict(t, key, out, recon, layer, refresh=dict(q, forced, period))"""
    from oracle_lib import Oracle
    h, w = frames[0][0].shape
    Oracle.lib().vp8o_set_conformant_stream(1 if conformant else 0)
    try:
        be = temporal_ref.oracle_backend(w, h, cfg.get("ssim_target", -1.0))
        drv = refresh_driver(be, w, h, layers, schedule, **cfg)
        rec, tl0 = [], -1
        for t, f in enumerate(frames):
            out = drv.encode_frame(*f, force_key=t in force_key)
            key = out is None
            layer = dict(drv.layer)
            tl0 += layer["temporal_id"] == 0
            layer["tl0_pic_idx"] = tl0 & 255
            recon = be.download_last() if layer["refresh"] in (temporal_ref.LAST, temporal_ref.ALL) else be.refresh_recon
            rec.append(dict(t=t, key=key, out=drv.last_key if key else out, recon=tuple(p.copy() for p in recon), layer=layer,
                            refresh=dict(drv.info)))
        be.close()
        return rec
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)
