"""Contents, segment data and reach for the tests that take the macroblock stage over the whole quantiser space
(test_quantiser_space_cpu.py, test_gpu_quantiser_space.py).  No GPU and no reference kernels in here: the restatement alone.

CONTENTS (64x48: twelve macroblocks, two workgroups of eight, the second partial; one 16x16 frame: a single macroblock).  A flat
reference makes the prediction independent of the vector the search picks, so the residual is the content's to choose (at the price of
one sign per frame); a frame against its inverse makes every residual at the zero vector +-255.
    flat_up / flat_down   flat 0 -> flat 255 and back: every first-order DC at +-2040, the second-order DC at the 16320 that tdiv's
                          comment allows (kernels_mb.hip), chroma DC 2040 over the smallest quantiser
    hadamard              flat 0 -> macroblocks whose sixteen 4x4 luma blocks are flat 0 or 255 by an outer product of two of the rows
                          ++++ ++-- +--+ +-+-: the second-order block has ONE large AC coefficient beside its DC
    pixels_inv            random single pixels -> their inverse: split macroblocks, large first-order AC
    squares_inv           random 4-pixel squares -> their inverse: split and whole macroblocks, split-macroblock luma DC at its bound
    flat_pixels           flat 0 -> random single pixels
    ramp128, squares128   a ramp / 4-pixel squares on flat 128: both signs of residual in one frame (for the segment loop)
    *_3refs               the inverse contents with GOLDEN and ALTREF of the same kind in use: select_reference picks among three nets
    one_mb                16x16, squares -> inverse

CASES: (tag, segment data[4][11], SSIM target).  (a) every index 0..127 in all four segments, no deltas; (b) the four delta sets of
+-15 in segment 0 at the indices that drive qi()'s clamp at both ends and across the tables, segments 1-3 with OTHER deltas that
nobody may read (GPU_kernels.cl:1396,1570 read SD[0]'s); (c) two ladders of indices with the targets that stop the segment loop
after one pass (0.5), somewhere (0.90, 0.97) and never (2.0)."""
import numpy as np

from pipeline import default_segments, run_inter_frame
from test_gpu_search_saturating import _binary

W, H = 64, 48
ROWS = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]])


def _flat(v, w=W, h=H):
    return (np.full((h, w), v, np.uint8), np.full((h // 2, w // 2), v, np.uint8), np.full((h // 2, w // 2), v, np.uint8))


def _inverse(f):
    return tuple(np.ascontiguousarray(255 - p) for p in f)


def _hadamard(rng):
    y = np.zeros((H, W), np.uint8)
    pats = rng.permutation(16)
    for k, (my, mx) in enumerate((a, b) for a in range(H // 16) for b in range(W // 16)):
        p = int(pats[k % 16]) if k else 5          # (the first macroblock: a pattern with a single AC coefficient in both directions)
        cells = (np.outer(ROWS[p >> 2], ROWS[p & 3]) > 0).astype(np.uint8) * 255
        y[my * 16:my * 16 + 16, mx * 16:mx * 16 + 16] = np.kron(cells, np.ones((4, 4), np.uint8))
    c = np.ascontiguousarray(y[::2, ::2])
    return y, c, c.copy()


def _ramp():
    y = ((np.add.outer(np.arange(H) * 5, np.arange(W) * 4)) % 256).astype(np.uint8)
    c = np.ascontiguousarray(y[::2, ::2])
    return y, c, np.ascontiguousarray(255 - c)


def _make_contents():
    rng = np.random.default_rng(24)
    c = {}
    lo, hi, mid = _flat(0), _flat(255), _flat(128)
    px1 = [_binary(rng, W, H, 1) for _ in range(3)]
    px4 = [_binary(rng, W, H, 4) for _ in range(3)]
    # name -> (cur, [LAST, GOLDEN, ALTREF], (use_golden, use_altref))
    c["flat_up"] = (hi, [lo, lo, lo], (0, 0))
    c["flat_down"] = (lo, [hi, hi, hi], (0, 0))
    c["hadamard"] = (_hadamard(rng), [lo, lo, lo], (0, 0))
    c["pixels_inv"] = (_inverse(px1[0]), [px1[0]] * 3, (0, 0))
    c["squares_inv"] = (_inverse(px4[0]), [px4[0]] * 3, (0, 0))
    c["flat_pixels"] = (_binary(rng, W, H, 1), [lo, lo, lo], (0, 0))
    c["ramp128"] = (_ramp(), [mid, mid, mid], (0, 0))
    c["squares128"] = (_binary(rng, W, H, 4), [mid, mid, mid], (0, 0))
    c["pixels_inv_3refs"] = (_inverse(px1[0]), px1, (1, 1))
    c["squares_inv_3refs"] = (_inverse(px4[0]), px4, (1, 1))
    one = _binary(rng, 16, 16, 4)
    c["one_mb"] = (_inverse(one), [one] * 3, (0, 0))
    return c


CONTENTS = _make_contents()
TABLE_CONTENTS = ["flat_up", "flat_down", "hadamard", "pixels_inv", "squares_inv", "flat_pixels"]
LOOP_CONTENTS = ["flat_up", "hadamard", "pixels_inv", "squares_inv", "ramp128", "squares128"]   # what the segment-loop figures are counted over
INVERSE_CONTENTS = ["pixels_inv", "squares_inv", "pixels_inv_3refs", "squares_inv_3refs"]

DELTA_SETS = {"plus": (15, 15, 15, 15, 15), "minus": (-15, -15, -15, -15, -15), "alt": (15, -15, 15, -15, 15), "alt_inv": (-15, 15, -15, 15, -15)}
CLAMP_INDICES = [q for q in range(128) if q % 8 in (0, 7)]       # 0, 7, 8, ..., 120, 127
LADDERS = {"ladder120": (0, 40, 80, 120), "ladder127": (15, 63, 100, 127)}
TARGETS = (0.5, 0.90, 0.97, 2.0)


def segments(qi, deltas=(0, 0, 0, 0, 0), junk=False):
    """segment data with the four indices `qi`, segment 0's five deltas, and (junk) deltas in segments 1-3 that nobody may read"""
    sd = default_segments(qi=tuple(qi))
    sd[:, 1:6] = 0
    sd[0, 1:6] = deltas
    if junk:
        for i in range(1, 4):
            sd[i, 1:6] = (7 * i, -3 * i, 5, -9, 11)
    return sd


def index_sweep(step=1):
    return [(f"q{q}", segments((q,) * 4), -1.0) for q in range(0, 128, step)]


def delta_sets():
    return [(f"q{q}_{name}", segments((q,) * 4, d, junk=True), -1.0) for q in CLAMP_INDICES for name, d in DELTA_SETS.items()]


def ladders(targets=TARGETS):
    return [(f"{name}_t{t}", segments(l, DELTA_SETS["alt" if name == "ladder120" else "alt_inv"], junk=True), t)
            for name, l in LADDERS.items() for t in targets]


_restated = {}


def restatement(name, case):
    """every stage output of the restatement for one content and case (kept: the reach and the live pin look at the same runs)"""
    tag, sd, target = case
    if (name, tag) not in _restated:
        from oracle_lib import Oracle
        cur, refs, (ug, ua) = CONTENTS[name]
        _restated[(name, tag)] = run_inter_frame(Oracle.stages(), cur, refs, sd, ug, ua, target)
    return _restated[(name, tag)]


def reach(pairs):
    """what a list of (content, case) reaches, from the restatement alone: the six maxima, the signs of the second-order DC, the
    values of MB_parts, the histogram of MB_segment_id and whether the filtered luma holds both 0 and 255"""
    r = dict(y2_dc=0, y2_dc_min=0, y2_dc_max=0, y2_ac=0, split_luma_dc=0, ac=0, chroma_ac=0, chroma_dc=0, parts=set(),
             segments=np.zeros(4, np.int64), recon_0_and_255=False, max_coefficient=0)
    for name, case in pairs:
        o = restatement(name, case)
        c, parts = o["MB_coeffs"].astype(np.int64), o["MB_parts"]
        whole, split = c[parts == 0], c[parts != 0]
        if len(whole):
            r["y2_dc_min"] = min(r["y2_dc_min"], int(whole[:, 24, 0].min()))
            r["y2_dc_max"] = max(r["y2_dc_max"], int(whole[:, 24, 0].max()))
            r["y2_ac"] = max(r["y2_ac"], int(np.abs(whole[:, 24, 1:]).max()))
            r["max_coefficient"] = max(r["max_coefficient"], int(np.abs(whole[:, 24]).max()))
        if len(split):
            r["split_luma_dc"] = max(r["split_luma_dc"], int(np.abs(split[:, :16, 0]).max()))
        r["ac"] = max(r["ac"], int(np.abs(c[:, :16, 1:]).max()))
        r["chroma_ac"] = max(r["chroma_ac"], int(np.abs(c[:, 16:24, 1:]).max()))
        r["chroma_dc"] = max(r["chroma_dc"], int(np.abs(c[:, 16:24, 0]).max()))
        r["parts"] |= set(int(p) for p in np.unique(parts))
        r["segments"] += np.bincount(o["MB_segment_id"], minlength=4)
        r["recon_0_and_255"] |= bool((o["recon_Y"] == 0).any() and (o["recon_Y"] == 255).any())
    r["y2_dc"] = max(-r["y2_dc_min"], r["y2_dc_max"])
    r["max_coefficient"] = max(r["max_coefficient"], r["split_luma_dc"], r["ac"], r["chroma_ac"], r["chroma_dc"])
    return r


def cpu_case_list():
    """(content, case) for the CPU file: (a) every index on three contents and every eighth on the rest; (b) every delta set at every
    clamp index on two contents, and on four more one delta set per index, in rotation; (c) on the six contents the segment-loop
    figures are counted over -- about 950 runs of 64x48"""
    full = ("flat_up", "pixels_inv", "squares_inv")
    pairs = [(n, c) for n in CONTENTS for c in index_sweep(1 if n in full else 8)]
    pairs += [(n, c) for n in ("hadamard", "squares_inv") for c in delta_sets()]
    for k, n in enumerate(("flat_down", "pixels_inv", "squares_inv_3refs", "one_mb")):
        pairs += [(n, c) for j, c in enumerate(delta_sets()) if j % 4 == (j // 4 + k) % 4]
    pairs += [(n, c) for n in LOOP_CONTENTS for c in ladders()]
    return pairs
