"""Temporal layers restated in Python from the TEXT of include/vp8hip_host.h (not from vp8host_temporal_step's C++): the rule, a
simulation of the three reference buffers on frame numbers (the closure property an SFU relies on), and the CPU oracle's frame loop
with the rule's reference sets and refreshes -- the expected bytes and reconstructions tests/test_gpu_temporal.py holds the native
driver to.  tests/test_temporal_cpu.py holds the host function and the host header coder to it without a GPU."""
import numpy as np

LAST, GOLDEN, NONE, ALL = 0, 1, 2, 3      # VP8HOST_REFRESH_*
GOLDEN_ONLY, REFRESH_NOTHING = 2, 3       # is_golden of an inter frame that refreshes GOLDEN only / nothing


def step(layers, p, ref_mask=3):
    """the rule -> dict(temporal_id, use_golden, refresh, layer_sync), or None where it refuses"""
    if layers not in (1, 2, 3) or p < 0:
        return None
    if p == 0:
        return dict(temporal_id=0, use_golden=0, refresh=ALL, layer_sync=0)
    if layers == 2 and p % 2 == 1:
        return dict(temporal_id=1, use_golden=0, refresh=NONE, layer_sync=1)
    if layers == 3 and p % 4 == 1:
        return dict(temporal_id=2, use_golden=0, refresh=NONE, layer_sync=1)
    if layers == 3 and p % 4 == 2:
        return dict(temporal_id=1, use_golden=0, refresh=GOLDEN, layer_sync=1)
    if layers == 3 and p % 4 == 3:
        g = ref_mask & 1
        return dict(temporal_id=2, use_golden=g, refresh=NONE, layer_sync=int(not g))
    return dict(temporal_id=0, use_golden=0, refresh=LAST, layer_sync=0)


def records(layers, keys, total, ref_mask=3):
    """the layer record of every frame of a stream whose key frames are the frame numbers in `keys` (frame 0 is one) -> list of dicts
    with p and tl0_pic_idx added"""
    out, p, tl0 = [], 0, -1
    for t in range(total):
        if t == 0 or t in keys:
            p = 0
        r = dict(step(layers, p, ref_mask), p=p, key=p == 0)
        if r["temporal_id"] == 0:
            tl0 += 1
        r["tl0_pic_idx"] = tl0 & 255
        out.append(r)
        p += 1
    return out


def simulate(recs, keep_tid):
    """Three buffers that hold frame numbers follow the refresh rule over the frames of temporal_id <= keep_tid -> {t: (searched
    buffers' contents as {buffer: (frame number, its temporal_id)})} for the frames kept"""
    buf = {LAST: None, GOLDEN: None, 2: None}
    seen = {}
    for t, r in enumerate(recs):
        if r["temporal_id"] > keep_tid:
            continue
        if r["key"]:
            seen[t] = {}
            buf = {LAST: (t, 0), GOLDEN: (t, 0), 2: (t, 0)}
            continue
        seen[t] = {b: buf[b] for b in ([LAST, GOLDEN] if r["use_golden"] else [LAST])}
        if r["refresh"] == LAST:
            buf[LAST] = (t, r["temporal_id"])
        elif r["refresh"] == GOLDEN:
            buf[GOLDEN] = (t, r["temporal_id"])
    return seen


# ---- the CPU oracle as the frame loop's backend ---------------------------------------------------------------------------------------
def oracle_backend(w, h, ssim_target=-1.0):
    """tests/oracle_lib.Oracle with the ending of a layered frame: loop_filter_refresh(GOLDEN): the filtered reconstruction becomes
    GOLDEN and LAST stays (the oracle's own rotation does the copy, as for a hidden frame's ALTREF); (NONE): it is kept aside for the
    test and LAST stays"""
    from oracle_lib import Oracle

    class TemporalOracle(Oracle):
        def loop_filter(self):
            super().loop_filter()
            self._last = tuple(p.copy() for p in self.download_last())

        def upload_last(self, y, u, v):
            super().upload_last(y, u, v)
            self._last = (np.ascontiguousarray(y).copy(), np.ascontiguousarray(u).copy(), np.ascontiguousarray(v).copy())

        def loop_filter_refresh(self, refresh):
            if refresh == LAST:
                return self.loop_filter()
            keep = self._last
            Oracle.loop_filter(self)                   # the filtered reconstruction is the oracle's LAST for a moment ...
            self.refresh_recon = tuple(p.copy() for p in self.download_last())
            if refresh == GOLDEN:                      # ... a transform with prev_is_golden = 1 copies it into GOLDEN; what it codes is thrown away
                self.inter_transform(1, 0, 0, 0)
            super().upload_last(*keep)                 # ... and LAST is what it was
            self._lf = dict(self._lf, recon_Y=keep[0], recon_U=keep[1], recon_V=keep[2])

    return TemporalOracle(w, h, ssim_target)


def layered_driver(backend, w, h, layers, **cfg):
    """vp8oclenc_amd.driver.InterPathDriver with frame_body's layered branch: references and ending from the rule, the lastqi ladder"""
    from vp8oclenc_amd.driver import InterPathDriver

    class TemporalDriver(InterPathDriver):
        p = 0
        layer = None

        def _key_frame(self, y, u, v):
            self.p = 1
            self.layer = step(layers, 0, self.ref_mask)
            return super()._key_frame(y, u, v)

        def encode_frame(self, y, u, v, force_key=False):
            g = self.gop.next()
            self.be.upload_current(y, u, v)
            if g.current_is_key or force_key:
                return self._key_frame(y, u, v)
            t = step(layers, self.p, self.ref_mask)
            sd = self.segments_for(y, False, False)
            self.be.set_segments(sd)
            self.be.inter_transform(g.prev_is_golden, g.prev_is_altref, t["use_golden"], 0)
            out = {"segments": sd, "use_golden": t["use_golden"], "use_altref": 0, "is_altref": 0}
            if self.check:
                replaced, new_ssim, min1 = self.be.check_ssim()
                out.update(replaced=replaced, new_SSIM=new_ssim, min_SSIM=min1)
                if min1 > np.float32(0.95):
                    sd = self.segments_for(y, False, False, update_filter=True)
                    self.be.set_segments(sd)
                    out["segments"] = sd
                if replaced > self.mbs // 6 or new_ssim < np.float32(self.ssim_target):
                    self.redone_as_key += 1
                    return self._key_frame(y, u, v)
            out.update(self.be.download_results(recon=True))
            if self.check:
                out["modes"], out["is_inter"] = self.be.download_intra()
            out["sharpness"] = self.sharpness
            self.be.prepare_filter_mask(want_nz=False)
            self.be.loop_filter_refresh(t["refresh"])
            self.gop.frame_done()
            self.inter_frames += 1
            self.layer = t
            self.p += 1
            return out

    return TemporalDriver(backend, w, h, **cfg)


def oracle_loop(frames, layers, conformant=False, force_key=(), **cfg):
    """The CPU oracle through the layered loop -> a list of records dict(t, key, out, recon, layer) in stream order: out = the frame's
    outputs as tests/bitstream_cases.expected_frame takes them, recon = the loop-filtered reconstruction whatever buffer it went to
    (or none), layer = the rule's word on the frame with tl0_pic_idx added."""
    from oracle_lib import Oracle
    h, w = frames[0][0].shape
    Oracle.lib().vp8o_set_conformant_stream(1 if conformant else 0)
    try:
        be = oracle_backend(w, h, cfg.get("ssim_target", -1.0))
        drv = layered_driver(be, w, h, layers, **cfg)
        rec, tl0 = [], -1
        for t, f in enumerate(frames):
            out = drv.encode_frame(*f, force_key=t in force_key)
            key = out is None
            layer = dict(drv.layer)
            tl0 += layer["temporal_id"] == 0
            layer["tl0_pic_idx"] = tl0 & 255
            recon = be.download_last() if layer["refresh"] in (LAST, ALL) else be.refresh_recon
            rec.append(dict(t=t, key=key, out=drv.last_key if key else out, recon=tuple(p.copy() for p in recon), layer=layer))
        rec[0]["redone_as_key"] = drv.redone_as_key
        be.close()
        return rec
    finally:
        Oracle.lib().vp8o_set_conformant_stream(0)


def record_bytes(rec, w, h, partitions):
    """The bytes of a record's frame.  A frame that refreshes LAST (or is a key frame) is one the reference knows: tests/bitstream_cases
    .expected_frame, first partition by the reference's own coder where it is built.  A GOLDEN-only or unreferenced frame has header bits
    the reference never writes: the coefficient partitions by the entropy oracle as for any frame, the first partition by the project's
    host coder with is_golden = 2 / 3 -- so for those frames a byte comparison holds the device coder to the host coder, and the judge
    independent of both is the decoder (tests/vp8_parse.py on the bits, tests/vp8_decode.py on conformant streams)."""
    from bitstream_cases import expected_frame
    refresh = rec["layer"]["refresh"]
    if refresh in (LAST, ALL):
        return expected_frame(w, h, rec["out"], rec["key"], partitions)
    from vp8oclenc_amd import bitstream
    flags = (0, GOLDEN_ONLY if refresh == GOLDEN else REFRESH_NOTHING, 0)
    real = bitstream.encode_header

    def with_flags(W, H, _flags, *a, **k):
        return real(W, H, flags, *a, **k)

    bitstream.encode_header = with_flags      # (expected_frame names the flags of an inter frame itself: (0, 0, is_altref))
    try:
        return expected_frame(w, h, rec["out"], False, partitions, use_reference=False)
    finally:
        bitstream.encode_header = real
