"""Hidden alternate reference frames without a GPU: vp8host_arf_filter_frame against the numpy restatement of include/vp8hip_host.h's
rule (tests/arf_ref.py) byte for byte, content that makes each branch of the rule occur, the division helper over every pair that can
occur, the hidden frame in the host bitstream, and a sequence with hidden frames from the CPU oracle's frame loop through the RFC 6386
decoder of tests/vp8_decode.py.  Everything is exact: no tolerances.  tests/test_gpu_arf.py holds the kernel and the native driver to
the same restatement and the same loop."""
import glob
import os

import numpy as np
import pytest

import arf_ref as ref
from vp8oclenc_amd import api, bitstream

SIZES = [(16, 16), (64, 48), (40, 24), (56, 40)]      # only the zero vector; interior and edge tiles; cut tiles
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "bitstream", "inter_*.npz")))


def same(got, want, what):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{what}: plane {name}: {len(bad)} samples differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} for {w[tuple(bad[0])]}"


# ---- 1. the host function against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", [0, 3, 6])
@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("w,h", SIZES)
def test_host_function_equals_the_restatement_byte_for_byte(w, h, n, strength):
    frames = ref.wild(w, h, n, seed=w + n)
    seen = [0, 0, 0]
    for centre in sorted({0, n // 2, n - 1}):
        want, ww, wv = ref.filter_frame(frames, centre, strength)
        got, gw, gv = api.arf_filter_frame(frames, centre, strength)
        same(got, want, f"centre {centre}")
        assert gw == ww and np.array_equal(gv, wv), centre
        assert sum(gw) == ((w + 15) // 16) * ((h + 15) // 16) * (n - 1)
        seen = [a + b for a, b in zip(seen, gw)]
        if n == 1:
            same(got, frames[0], "n = 1 returns the centre frame")
    if w == 16:
        assert not gv.any()      # a picture of one tile: only the zero vector lies inside the extended picture
    if n == 7 and w > 16:
        assert seen[2] > 0 and seen[0] > 0      # (the frames were chosen to make matched and unmatched tiles)


def test_bad_arguments_are_refused():
    f = ref.wild(32, 16, 2)
    for bad in (dict(centre=2), dict(centre=-1), dict(strength=7), dict(strength=-1)):
        with pytest.raises(ValueError):
            api.arf_filter_frame(f, **dict(dict(centre=0, strength=3), **bad))
    with pytest.raises(ValueError):
        api.arf_filter_frame(f * 4, 0, 3)      # eight frames
    odd = [(np.zeros((16, 18), np.uint8)[:, :17], np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8))]
    with pytest.raises(ValueError):
        api.arf_filter_frame(odd, 0, 3)


# ---- 2. content -------------------------------------------------------------------------------------------------------------------------
def _tiles(w, h):
    return [(tx, ty) for ty in range((h + 15) // 16) for tx in range((w + 15) // 16)]


def test_a_translation_inside_the_range_is_found_and_filters_to_the_centre():
    w, h, n, c, step = 96, 64, 3, 1, (4, -2)
    frames = ref.translating(w, h, n, step)
    out, weights, vec = api.arf_filter_frame(frames, c, 3)
    exact = 0
    for t, (tx, ty) in enumerate(_tiles(w, h)):
        whole = True
        for k in range(n):
            dx, dy = (c - k) * step[0], (c - k) * step[1]      # frame k shows the texture k * step further on: the centre's block lies (c - k) * step away in it
            ok = 0 <= tx * 16 + dx and tx * 16 + dx + 16 <= w and 0 <= ty * 16 + dy and ty * 16 + dy + 16 <= h
            if ok:
                assert tuple(vec[t, k]) == (dx, dy), (tx, ty, k, tuple(vec[t, k]))
            whole &= ok
        if whole:      # every frame matched without an error: weights 16 * 2 on equal samples
            exact += 1
            assert np.array_equal(out[0][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16], frames[c][0][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16])
            assert np.array_equal(out[1][ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8], frames[c][1][ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8])
    assert exact >= 4 and weights[2] >= 2 * exact


def test_a_translation_outside_the_range_has_weight_zero():
    w, h = 64, 48
    frames = ref.translating(w, h, 3, (14, 12))
    out, weights, _ = api.arf_filter_frame(frames, 1, 3)
    assert weights == [2 * 12, 0, 0]
    same(out, frames[1], "weight 0 everywhere: the centre")


def test_noise_on_a_still_picture_is_reduced():
    frames, clean = ref.noisy_still(64, 48, 7, amplitude=6)
    out, weights, vec = api.arf_filter_frame(frames, 3, 3)
    assert weights[2] == 6 * 12 and not vec.any()
    for p in range(3):
        assert not np.array_equal(out[p], frames[3][p])
        err = lambda a: int(((a.astype(np.int64) - clean[p]) ** 2).sum())
        assert err(out[p]) < err(frames[3][p]), (p, err(out[p]), err(frames[3][p]))


def test_a_scene_cut_inside_the_window_is_left_out():
    w, h = 64, 48
    a, b = ref.translating(w, h, 3, (2, 0), seed=4), ref.translating(w, h, 2, (2, 0), seed=40)
    out, weights, _ = api.arf_filter_frame(a + b, 1, 3)
    alone, wa, _ = api.arf_filter_frame(a, 1, 3)
    assert weights[0] == wa[0] + 2 * 12      # both frames behind the cut: weight 0 in every tile
    same(out, alone, "the frames behind the cut do not count")


def test_flat_frames_tie_and_the_zero_vector_wins():
    w, h = 48, 32
    frames = [tuple(np.full(s, v, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))) for v in (100, 103, 98)]
    out, weights, vec = api.arf_filter_frame(frames, 1, 3)
    assert not vec.any() and weights == [0, 0, 12]
    want, _, wv = ref.filter_frame(frames, 1, 3)
    same(out, want, "flat")
    assert not wv.any()


# ---- 3. the division ----------------------------------------------------------------------------------------------------------------------
def test_the_reciprocal_multiply_is_exact_for_every_pair_that_can_occur():
    acc = np.arange(65536, dtype=np.uint32)      # acc is at most 255 * count, below 65536: every acc below 65536, for every count of the rule
    for count in range(32, 225):
        c = np.full(65536, count, np.uint32)
        got = api.arf_round_divide(acc, c)
        assert np.array_equal(got, (acc + count // 2) // count), count


# ---- 4. the hidden frame in the host bitstream --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_a_hidden_frame_parses_as_one_and_an_ordinary_frame_keeps_its_bytes(path):
    import vp8_parse as vp
    z = np.load(path)
    opt = lambda k: np.ascontiguousarray(z[k]) if k in z.files else None
    W, H = int(z["W"]), int(z["H"])

    def header(flags):
        return bitstream.encode_header(W, H, flags, z["sd"], z["seg"], z["nz"], z["probs"], z["denom"], int(z["skip_prob"]), ref_frame=opt("ref_frame"),
                                       parts=opt("parts"), vectors=opt("vectors"), is_inter=opt("is_inter"), modes=opt("modes"),
                                       replaced=int(z["replaced"]), sharpness=int(z["sharpness"]), partitions_log2=int(z["partitions_log2"]))[0]

    flags = tuple(int(x) for x in z["flags"])
    assert np.array_equal(header(flags), z["header"])      # the reference's bytes, as before
    P = 1 << int(z["partitions_log2"])
    tokens = [np.zeros(4096, np.uint8)] * P      # (no coefficient partitions in the fixture: zeros decode to some tokens, the same for both)
    frames = {}
    for name, fl in (("shown", (0, 0, 1)), ("hidden", (0, 0, api.ALTREF_HIDDEN))):
        hdr = header(fl)
        st = vp.StreamState()
        st.width, st.height = W, H      # (what a key frame would have set)
        frames[name] = (hdr, vp.parse_frame(bitstream.gather_frame(hdr, tokens).tobytes(), st))
    assert len(frames["shown"][0]) == len(frames["hidden"][0])
    shown, hidden = frames["shown"][1], frames["hidden"][1]
    assert (hidden.key, hidden.show, hidden.refresh_last, hidden.refresh_altref, hidden.refresh_golden, hidden.copy_to_golden, hidden.copy_to_altref) == \
           (0, 0, 0, 1, 0, 0, 0)
    assert (shown.show, shown.refresh_last, shown.refresh_altref) == (1, 1, 1)
    for k in ("ref_frame", "mv_mode", "mvs", "is_inter", "segment_id", "skip"):      # everything else stays as an inter frame has it
        assert np.array_equal(getattr(shown, k), getattr(hidden, k)), k


# ---- 5. a sequence with hidden frames through the decoder ----------------------------------------------------------------------------------
def test_an_oracle_sequence_with_hidden_frames_decodes_to_the_oracle_reconstruction():
    import vp8_decode
    w, h, total, gop, period = 64, 48, 12, 12, 4
    frames = ref.noisy_pan(w, h, total, seed=6)
    placement = ref.schedule(total, gop, period)
    assert sorted(placement) == [0, 4, 8] and placement[0][3] == "after" and placement[4][3] == "before"
    recs = ref.oracle_loop(frames, placement, strength=3, conformant=True, gop_size=gop, altref_range=5, qi_min=10, qi_max=60)
    assert [r["kind"] for r in recs].count("hidden") == 3
    dec = vp8_decode.Decoder()
    altref_chosen = 0
    for i, r in enumerate(recs):
        last_before = dec.ref.get(1) if hasattr(dec, "ref") and dec.ref else None
        f, planes = dec.decode(ref.record_bytes(r, w, h, 2))
        same(planes, r["recon"], f"record {i} ({r['kind']} at frame {r['t']})")
        if r["kind"] == "hidden":
            assert (f.show, f.refresh_last, f.refresh_altref, f.refresh_golden) == (0, 0, 1, 0)
            assert dec.ref[1] is last_before, "a hidden frame leaves the decoder's LAST alone"
            assert dec.ref[3] is planes
            assert sum(r["weights"][1:]) > 0
        elif not r["key"]:
            assert f.show == 1 and f.refresh_last == 1
            altref_chosen += int((f.ref_frame[f.is_inter.astype(bool)] == 3).sum())
    assert altref_chosen > 0      # (and the shown frames use it)


@pytest.mark.parametrize("placement", [{0: (0, 4, 3, "after"), 6: (6, 3, 2, "after")}, {3: (1, 5, 3, "after"), 5: (3, 3, 2, "before")},
                                       {2: (0, 5, 2, "before"), 3: (1, 5, 3, "after"), 4: (2, 4, 2, "before")}],
                         ids=["behind key frames", "behind a scheduled alt-ref", "two in a row"])
@pytest.mark.parametrize("ref_mask", [3, 0])
def test_the_rotation_owed_is_applied_once_in_the_oracle_loop(placement, ref_mask):
    """hidden frames where the rotation can go wrong (GOP of 6, scheduled alt-ref every 3): had the shown frame behind a hidden one
    applied the rotation again, the loop's ALTREF would be LAST while the decoder's is the hidden frame, and the reconstructions part"""
    import vp8_decode
    w, h, total = 64, 48, 9
    frames = ref.noisy_pan(w, h, total, seed=9)
    recs = ref.oracle_loop(frames, placement, strength=3, conformant=True, gop_size=6, altref_range=3, ref_mask=ref_mask, qi_min=10, qi_max=60)
    dec = vp8_decode.Decoder()
    for i, r in enumerate(recs):
        f, planes = dec.decode(ref.record_bytes(r, w, h, 1))
        same(planes, r["recon"], f"record {i} ({r['kind']} at frame {r['t']})")
        assert f.show == (r["kind"] == "shown")
    assert sum(r["key"] for r in recs) == 2 and sum(r["kind"] == "hidden" for r in recs) == len(placement)
