"""The expected result of an inter frame coded under a segment map (vp8hip_set_segment_mode), assembled from the oracle's stage
functions in the stage order of tests/pipeline.py.  An inter macroblock's transform is local to the macroblock, so:
  1. the searches and the predictors run once;
  2. the one-pass transform (ssim_target = -1: every macroblock takes the first pass, segment 3, and no other) runs four times, run s
     with segment 3's y_ac_i replaced by the ladder's entry s -- the quantiser deltas are the frame's, row 0's, in every run;
  3. each macroblock's coefficients, pre-filter reconstruction, SSIM and non-zero count come from run map[mb];
  4. prepare_filter_mask's mask and the loop filter run on the assembled frame with MB_segment_id = map and the unmodified data.
Test infrastructure."""
from __future__ import annotations

import numpy as np

from pipeline import pyramid


def _searches_and_predictors(st, cur, refs, use):
    Y, U, V = cur
    H, W = Y.shape
    mbs = (W // 16) * (H // 16)
    b8 = mbs * 4
    net_width = (W // 16) * 2
    cur_pyr = pyramid(st, Y)
    nets1, bdiffs = [], []
    for r in range(3):
        net = [np.zeros((b8, 2), np.int16), np.zeros((b8, 2), np.int16)]
        bd = np.full(b8, 0x7FFFFFFF, np.int32)
        if use[r]:
            ref_pyr = pyramid(st, refs[r][0])
            src = 0
            for l in range(4, -1, -1):
                st.luma_search_1step(cur_pyr[l], ref_pyr[l], net[src], net[src ^ 1], net_width, W >> l, H >> l, 1 << l)
                src ^= 1
            st.luma_search_2step(Y, np.ascontiguousarray(refs[r][0]), net[1], net[0], bd, W, H)
        nets1.append(net[0])
        bdiffs.append(bd)
    MB_ref = np.zeros(mbs, np.int32)
    MB_vec = np.zeros((mbs, 4, 2), np.int16)
    MB_parts = np.zeros(mbs, np.int32)
    MB_SSIM = np.zeros(mbs, np.float32)
    st.select_reference(nets1[0], nets1[1], nets1[2], bdiffs[0], bdiffs[1], bdiffs[2], MB_ref, MB_vec, W, H, use[1], use[2])
    st.pack_8x8_into_16x16(MB_vec, MB_parts, MB_SSIM, mbs)
    planes = [(Y, W, H), (U, W // 2, H // 2), (V, W // 2, H // 2)]
    pred = [np.zeros_like(p[0]) for p in planes]
    resid = [np.zeros(p[0].shape, np.int16) for p in planes]
    for r in range(3):
        if not use[r]:
            continue
        for p, (pl, w, h) in enumerate(planes):
            st.prepare_predictors_and_residual(np.ascontiguousarray(pl), np.ascontiguousarray(refs[r][p]), pred[p], resid[p], MB_ref, MB_vec, w, h, p, r)
    return planes, pred, resid, MB_ref, MB_vec, MB_parts, MB_SSIM


def _one_pass_transform(st, planes, pred, resid, MB_parts, MB_SSIM0, sd):
    """the transform loop of pipeline.run_inter_frame at ssim_target = -1 on the given segment data"""
    (Y, W, H), (U, _, _), (V, _, _) = planes
    mbs = (W // 16) * (H // 16)
    sd = np.ascontiguousarray(sd, np.int32).reshape(-1)
    MB = np.zeros((mbs, 25, 16), np.int16)
    MB_seg = np.zeros(mbs, np.int32)
    MB_SSIM = MB_SSIM0.copy()
    recon = [np.zeros_like(p[0]) for p in planes]
    metric = [np.zeros(mbs, np.float32) for _ in range(3)]
    for seg in range(3, -1, -1):
        for p, (pl, w, h) in enumerate(planes):
            st.dct4x4(resid[p], MB, MB_seg, MB_parts, MB_SSIM, w, h, sd, seg, -1.0, p)
        st.wht4x4_iwht4x4(MB, MB_seg, MB_parts, sd, seg, mbs)
        for p, (pl, w, h) in enumerate(planes):
            st.idct4x4(recon[p], pred[p], MB, MB_seg, MB_parts, w, h, sd, seg, p)
        st.count_SSIM(np.ascontiguousarray(Y), recon[0], MB_seg, metric[0], W, H, seg, 16)
        st.count_SSIM(np.ascontiguousarray(U), recon[1], MB_seg, metric[1], W // 2, H // 2, seg, 8)
        st.count_SSIM(np.ascontiguousarray(V), recon[2], MB_seg, metric[2], W // 2, H // 2, seg, 8)
        st.gather_SSIM(metric[0], metric[1], metric[2], MB_SSIM, mbs)
    assert (MB_seg == 3).all()      # one pass, the first
    nz = np.zeros(mbs, np.int32)
    mask = np.zeros(mbs, np.int32)
    st.prepare_filter_mask(MB, nz, MB_parts, mask, W, H)
    return MB, MB_SSIM, recon, nz, mask


def run_mapped_inter_frame(st, cur, refs, sd, use_golden, use_altref, seg_map) -> dict:
    """cur = (Y, U, V); refs = [(Y, U, V)] * 3 (LAST, GOLDEN, ALTREF); sd = segment_data[4][11]; seg_map[MBs] in 0..3"""
    Y, U, V = (np.ascontiguousarray(p) for p in cur)
    H, W = Y.shape
    mbw = W // 16
    mbs = mbw * (H // 16)
    seg_map = np.asarray(seg_map).reshape(-1).astype(np.int32) & 3
    assert seg_map.size == mbs
    sd = np.ascontiguousarray(sd, np.int32).reshape(4, 11)
    use = [1, int(use_golden), int(use_altref)]
    planes, pred, resid, MB_ref, MB_vec, MB_parts, MB_SSIM0 = _searches_and_predictors(st, (Y, U, V), refs, use)
    MB = np.zeros((mbs, 25, 16), np.int16)
    MB_SSIM = np.zeros(mbs, np.float32)
    nz = np.zeros(mbs, np.int32)
    mask = np.zeros(mbs, np.int32)
    recon = [np.zeros_like(p[0]) for p in planes]
    for s in range(4):
        pick = np.nonzero(seg_map == s)[0]
        if not pick.size:
            continue
        sd_s = sd.copy()
        sd_s[3, 0] = sd[s, 0]
        MB_s, SSIM_s, recon_s, nz_s, mask_s = _one_pass_transform(st, planes, pred, resid, MB_parts, MB_SSIM0, sd_s)
        MB[pick], MB_SSIM[pick], nz[pick], mask[pick] = MB_s[pick], SSIM_s[pick], nz_s[pick], mask_s[pick]
        for mb in pick:
            x, y = (mb % mbw) * 16, (mb // mbw) * 16
            recon[0][y:y + 16, x:x + 16] = recon_s[0][y:y + 16, x:x + 16]
            for p in (1, 2):
                recon[p][y // 2:y // 2 + 8, x // 2:x // 2 + 8] = recon_s[p][y // 2:y // 2 + 8, x // 2:x // 2 + 8]
    filt = [r.copy() for r in recon]
    sdf = np.ascontiguousarray(sd.reshape(-1))
    st.loop_filter_frame(filt[0], seg_map, mask, sdf, W, H, 16)
    st.loop_filter_frame(filt[1], seg_map, mask, sdf, W // 2, H // 2, 8)
    st.loop_filter_frame(filt[2], seg_map, mask, sdf, W // 2, H // 2, 8)
    return dict(MB_reference_frame=MB_ref, MB_vectors=MB_vec, MB_parts=MB_parts, MB_SSIM=MB_SSIM, MB_coeffs=MB, MB_segment_id=seg_map,
                MB_non_zero_coeffs=nz, mb_mask=mask, prefilter_Y=recon[0], prefilter_U=recon[1], prefilter_V=recon[2],
                recon_Y=filt[0], recon_U=filt[1], recon_V=filt[2])
