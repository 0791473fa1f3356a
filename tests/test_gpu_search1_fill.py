"""The batched whole-pel search in its filled loop form (k_search1_plr_b: 51 blocks x 5 lanes per workgroup of 256 lanes, blocks numbered across the
workgroup, the minimum over a block's lanes through LDS, the metric's B operand in row order: csrc/s1_fill_layout.h, kernels_me.hip) against the
CPU oracle, bit for bit, at the smallest shapes where the new map can go wrong (level-0 blocks; the coarser levels have a quarter each):
    64x48    48: less than one workgroup (12 at level 1)
    176x144  396 = 7 x 51 + 39: a ragged last workgroup, block rows of 22 cut through workgroups
    272x48   204 = 4 x 51: an exact multiple
    320x192  960 = 18 x 51 + 42
One launch per shape holds four members: three cut from a panned texture with 1, 2 and 3 enabled references and different content and motion --
the pans point out of the frame at every edge, so out-of-frame candidates and the slots whose lanes lie in two waves (12, 25, 38) carry real
decisions -- and one of nearly unrelated noise frames with three references (the content of the `ushort cost wrap-around' case of
test_gpu_refcl.py and test_gpu_parity.py).  At these sizes a launch picks
the short-wave form by itself; VP8HIP_S1_SPLIT=0 forces the loop form on all five levels.  The switch is read once per process, so this file runs
as a program in a process of its own, once for all shapes (the cases below read what it printed).  The nets the device keeps are compared: the
level-0 net and the quarter-pel net and costs made from it; the nets of levels 4..1 are overwritten on the way down (two nets, ping-pong) and are
held through the level-0 vectors that descend from them.
The three-reference panned member also runs as a batch of ONE, per shape (grid z = 1).
Parent vectors at the int16 extremes: no content of these sizes produces them (when nothing is accepted a level hands down at most about the frame's
width), so the (int16_t) wraps of search1_block are driven directly.  On the same four members, with their pyramids standing, single levels of the
batched search (2, 1 and 0: vp8hip_debug_search1_batch, one launch_search1_batch each) run over WRITTEN source nets: in the parent cells a level
reads the components are 32767, -32768 (0x8000), -32767, 32766, -32766 or +-16384 along one axis, along both, or a few pixels both ways, so
that cy + v0y + (j - 2) and xb + i pass int16 for some blocks (at level 0: above it the parent is divided by the level's pixel rate first and only
the vector handed down, (v0 - c) * rate, can wrap), lie out of the frame for others and in it for the rest.  The oracle's luma_search_1step runs over the same planes and
nets; every block's cell must agree, and the child counts what the nets reach (extreme parents, blocks whose candidate positions pass int16, vectors
that leave the level farther out than the frame is wide), which the test asserts to be there.
The row-order operand itself is pinned through its tap (vp8hip_debug_weight_mfma_rows) on the blocks k_weight_tap_mfma is held on.
Run with `pytest -m gpu`."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

from oracle_lib import Oracle
from pipeline import default_segments
from vp8oclenc_amd import api
from vp8oclenc_amd.synth import noise_frames

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (176, 144), (272, 48), (320, 192)]
FLAGS = [(0, 0), (1, 0), (1, 1), (1, 1)]      # (use_golden, use_altref) per member: 1, 2 and 3 references; the noise member 3
# per panned member: where the LAST, GOLDEN and ALTREF sources are cut from the canvas relative to the current frame (x, y)
PANS = [[(5, 3), (-6, -4), (7, -5)], [(-4, 6), (6, 2), (-3, -7)], [(3, -6), (-7, 5), (-5, -2)]]
STRADDLING = (12, 25, 38)
MARGIN = 16


def _panned(W, H, seed, pans):
    """[LAST, GOLDEN, ALTREF sources, current]: windows of one textured canvas (smooth patches of 4 pixels + fine noise), the current at pan (0, 0)"""
    rng = np.random.default_rng(seed)
    hh, ww = H + 2 * MARGIN, W + 2 * MARGIN
    coarse = rng.integers(40, 216, size=(hh // 4 + 1, ww // 4 + 1))
    canvas = np.kron(coarse, np.ones((4, 4), np.int64))[:hh, :ww] + rng.integers(-20, 21, size=(hh, ww))
    canvas = np.clip(canvas, 0, 255).astype(np.uint8)

    def cut(dx, dy):
        y = np.ascontiguousarray(canvas[MARGIN + dy:MARGIN + dy + H, MARGIN + dx:MARGIN + dx + W])
        c = np.ascontiguousarray(y[::2, ::2])
        return y, c, np.ascontiguousarray(255 - c)
    return [cut(*p) for p in pans] + [cut(0, 0)]


def _frames(W, H):
    out = [_panned(W, H, 7000 + W + i, PANS[i]) for i in range(3)]
    nf = noise_frames(W, H, 23)
    return out + [[nf[0], nf[1], nf[0], nf[1]]]


def _prepare(be, frames):
    """frames[1] GOLDEN, frames[2] ALTREF, frames[0] LAST through the reference's own rotation rules; frames[3] is the current frame"""
    be.upload_last(*frames[1])
    be.upload_current(*frames[3])
    be.inter_transform(1, 0, 0, 0)
    be.loop_filter()
    be.upload_last(*frames[2])
    be.upload_current(*frames[3])
    be.inter_transform(0, 1, 0, 0)
    be.loop_filter()
    be.upload_last(*frames[0])
    be.upload_current(*frames[3])


@functools.lru_cache(maxsize=None)
def oracle_nets(W, H):
    """per member {(reference, what): array}, from the CPU oracle alone; computed once per shape"""
    res = []
    sd = default_segments()
    for frames, flags in zip(_frames(W, H), FLAGS):
        o = Oracle(W, H)
        o.set_segments(sd)
        _prepare(o, frames)
        o.inter_transform(0, 0, *flags)
        nets = {}
        for r in range(3):
            if r and not flags[r - 1]:
                continue
            nets[(r, "quarter-pel net")] = np.array(o.net(r, 1))
            nets[(r, "level-0 net")] = np.array(o.net(r, 2))
            nets[(r, "bdiff")] = np.array(o.bdiff(r))
        res.append(nets)
        o.close()
    return res


def content_report(W, H):
    """what the content reaches, from the oracle: (moving blocks at the frame's four edges, moving blocks in straddling slots, extreme component of
    the noise member's level-0 vectors, its largest winning quarter-pel cost)"""
    want = oracle_nets(W, H)
    bw, bh = W // 8, H // 8
    edges, straddle = 0, 0
    for nets in want[:3]:
        grid = np.asarray(nets[(0, "level-0 net")], np.int16).reshape(bh, bw, 2)      # a cell per 8x8 block, row by row
        moving = np.abs(grid).sum(axis=2) > 0
        edges += int(moving[0].sum() + moving[-1].sum() + moving[:, 0].sum() + moving[:, -1].sum())
        flat = moving.reshape(-1)
        straddle += int(sum(flat[b] for b in range(bw * bh) if b % 51 in STRADDLING))
    n = np.asarray(want[3][(0, "level-0 net")], np.int16)
    return edges, straddle, int(np.abs(n.astype(np.int32)).max()), int(np.asarray(want[3][(0, "bdiff")]).max())


def _differences(W, H, which=None, extremes=None):
    """[(member, reference, what, how many)] where the device's nets are not the oracle's: the four members in one launch, or member `which` as a
    batch of one (grid z = 1)"""
    idx = list(range(len(FLAGS))) if which is None else [which]
    n = len(idx)
    FLAGS_ = [FLAGS[i] for i in idx]
    want = [oracle_nets(W, H)[i] for i in idx]
    all_frames = [_frames(W, H)[i] for i in idx]
    sd = default_segments()
    members = [api.Vp8Hip(W, H) for _ in range(n)]
    lib = api.load_library()
    hb = C.c_void_p()
    bad = []
    try:
        for m, frames in zip(members, all_frames):
            m.set_segments(sd)
            _prepare(m, frames)
        lib.vp8hip_batch_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
        lib.vp8hip_batch_inter_transform.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 5
        lib.vp8hip_batch_destroy.argtypes = [C.c_void_p]
        lib.vp8hip_batch_destroy.restype = None
        assert lib.vp8hip_batch_create(C.byref(hb), (C.c_void_p * n)(*[m.h for m in members]), n) == 0
        ints = lambda v: (C.c_int * n)(*v)
        assert lib.vp8hip_batch_inter_transform(hb, None, ints([0] * n), ints([0] * n), ints([f[0] for f in FLAGS_]), ints([f[1] for f in FLAGS_])) == 0
        api.device_synchronize()
        for i, flags in enumerate(FLAGS_):
            for r in range(3):
                if r and not flags[r - 1]:
                    continue
                for name, tap in (("level-0 net", api.DBG_NET2), ("quarter-pel net", api.DBG_NET1), ("bdiff", api.DBG_BDIFF)):
                    got = np.asarray(members[i].debug(tap, r))
                    if not np.array_equal(got, want[i][(r, name)]):
                        bad.append((idx[i], r, name, int((got != want[i][(r, name)]).sum())))
        if extremes is not None:
            extremes += _extreme_differences(W, H, members, lib)
    finally:
        if hb:
            lib.vp8hip_batch_destroy(hb)
        for m in members:
            m.close()
    return bad


EXTREMES = (32767, -32768, -32767, 32766, -32766, 16384, -16384)
EXTREME_LEVELS = (2, 1, 0)


def _extreme_net(W, H, level, seed):
    """a source net for one level: (b8, 2) int16, cell (by * net_width + bx) = the vector of block (bx, by) of level + 1.  Written in the coarser
    level's block grid only: the cells beyond it are read but never written by a search, and the device reads them as the zeros the reference
    resets them to"""
    rng = np.random.default_rng(seed)
    net_width, b8 = W // 8, (W // 8) * (H // 8)
    pbw, pbh = (W >> (level + 1)) // 8, (H >> (level + 1)) // 8
    net = np.zeros((b8, 2), np.int16)
    for c in range(pbw * pbh):      # cell c: every third a few pixels both ways, every fifth extreme both ways, the others extreme along one axis
        bx, by = c % pbw, c // pbw
        for k in range(2):
            extreme = c % 3 != 2 and (c % 5 == 0 or k == c % 2)
            net[by * net_width + bx, k] = EXTREMES[(c + k + seed) % len(EXTREMES)] if extreme else int(rng.integers(-3, 4)) << level
    return net, pbw * pbh


def _extreme_reach(W, H, level, nets, outs):
    """(parent components at +-32767 / -32768 among the cells the level reads, blocks one of whose 25 candidate positions passes int16 before the
    cast, block vectors coming out longer than the frame is wide) over the given source nets and the oracle's results"""
    rate, net_width = 1 << level, W // 8
    bw, bh = (W >> level) // 8, (H >> level) // 8
    ext = wrap = far = 0
    for net, out in zip(nets, outs):
        for by in range(bh):
            for bx in range(bw):
                pv = net[(by >> 1) * net_width + (bx >> 1)].astype(np.int64)
                ext += int(np.isin(pv, (32767, -32768, -32767)).sum())
                v0 = np.sign(pv) * (np.abs(pv) // rate)          # the division truncates toward zero
                lo, hi = np.array([8 * bx, 8 * by]) + v0 - 2, np.array([8 * bx, 8 * by]) + v0 + 2
                wrap += int((lo < -32768).any() or (hi > 32767).any())
                far += int((np.abs(out[by * net_width + bx].astype(np.int64)) > max(W, H)).any())
    return ext, wrap, far


def _extreme_differences(W, H, members, lib):
    """per level [(level, (differences), (reach))]: one level of the batched search over written source nets against the oracle's luma_search_1step
    on the same planes and nets.  The members' pyramids stand (the batched inter_transform has run)"""
    st = Oracle.stages()
    n = len(FLAGS)
    use = [[1, f[0], f[1]] for f in FLAGS]
    lib.vp8hip_debug_search1_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    net_width, b8 = W // 8, (W // 8) * (H // 8)
    res = []
    for level in EXTREME_LEVELS:
        src, dst, cells = {}, {}, 0
        for i in range(n):
            for r in range(3):
                if use[i][r]:
                    src[(i, r)], cells = _extreme_net(W, H, level, 100000 * level + 1000 * i + 10 * r + W)
                    dst[(i, r)] = np.full((b8, 2), 0x5555, np.int16)
        if not cells:
            continue          # (no block of the coarser level: nothing to read)
        ptr = lambda d: (C.c_void_p * (3 * n))(*[d[(i, r)].ctypes.data if (i, r) in d else None for i in range(n) for r in range(3)])
        ints = lambda v: (C.c_int * n)(*v)
        rc = lib.vp8hip_debug_search1_batch((C.c_void_p * n)(*[m.h for m in members]), n, ints([f[0] for f in FLAGS]), ints([f[1] for f in FLAGS]), level, ptr(src), ptr(dst))
        assert rc == 0, rc
        bw, bh = (W >> level) // 8, (H >> level) // 8
        block_cells = np.array([by * net_width + bx for by in range(bh) for bx in range(bw)])
        bad, nets, outs = [], [], []
        for (i, r), s_net in src.items():
            cur = np.ascontiguousarray(members[i].debug(api.DBG_PYRAMID, 3, level))
            ref = np.ascontiguousarray(members[i].debug(api.DBG_PYRAMID, r, level))
            want = np.zeros((b8, 2), np.int16)
            st.luma_search_1step(cur, ref, s_net, want, net_width, W >> level, H >> level, 1 << level)
            diff = int((dst[(i, r)][block_cells] != want[block_cells]).any(axis=1).sum())
            if diff:
                bad.append((i, r, diff))
            nets.append(s_net)
            outs.append(want)
        res.append((level, bad, _extreme_reach(W, H, level, nets, outs)))
    return res


def _extreme_line(W, H, level):
    return f"{W}x{H} extreme parents, level {level}: differences: "


def _line(W, H, way="batch of 4"):
    return f"{W}x{H} {way}: differences: "


ONE = 2      # the member that also runs as a batch of one: three references, panned content


@functools.lru_cache(maxsize=None)
def _child():
    """this file as a program with the loop form forced on every level: its output, once"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, VP8HIP_S1_SPLIT="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_content_moves_at_the_edges_and_in_the_straddling_slots(W, H):
    """on the CPU, from the oracle: the content does what it is here for"""
    edges, straddle, extreme, cost = content_report(W, H)
    print(f"{W}x{H}: {edges} moving edge blocks, {straddle} moving blocks in slots {STRADDLING}; noise member: extreme vector component {extreme}, "
          f"largest winning cost {cost}")
    assert edges > 0 and straddle > 0


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_filled_loop_form_leaves_the_oracles_nets(W, H):
    out = _child()
    assert _line(W, H) + "[]" in out, out[-3000:]


@pytest.mark.parametrize("W,H", SHAPES)
def test_a_batch_of_one_leaves_the_oracles_nets(W, H):
    out = _child()
    assert _line(W, H, "batch of 1") + "[]" in out, out[-3000:]


@pytest.mark.parametrize("W,H", SHAPES)
def test_parent_vectors_at_the_int16_extremes_give_the_oracles_vectors(W, H):
    """levels 1 and 0 in every shape (level 2 too where the level above it has a block): the nets do reach the extremes -- and at level 0, where the
    parent is not divided, candidate positions that pass int16 --, and every block's vector is the oracle's"""
    out = _child()
    import re
    levels = [int(l) for l in re.findall(re.escape(f"{W}x{H} extreme parents, level ") + r"(\d)", out)]
    assert set(levels) >= {1, 0}, out[-3000:]
    for level in levels:
        m = re.search(re.escape(_extreme_line(W, H, level)) + r"(\[.*?\]); reach: (\d+) extreme parent components, (\d+) blocks whose candidates pass int16, (\d+) vectors out beyond the frame", out)
        assert m, out[-3000:]
        assert m.group(1) == "[]", m.group(0)
        assert int(m.group(2)) > 0 and int(m.group(4)) > 0, m.group(0)
        assert int(m.group(3)) > 0 or level > 0, m.group(0)


def test_block_match_metric_row_order_form_vs_oracle():
    """the blocks test_gpu_metric_mfma.py holds k_weight_tap_mfma on -- 200k random difference blocks of every amplitude plus the extreme
    sign-pattern blocks --, every lane of the tap on a different one, through the row-order A operand"""
    rng = np.random.default_rng(11)
    blocks = [rng.integers(-a, a + 1, size=(40000, 16)) for a in (1, 4, 32, 128, 255)]
    ext = []
    for s0 in (-255, 255):
        for pat in range(64):
            rows = [(1 if (pat >> r) & 1 else -1) for r in range(4)]
            cols = [(1 if (pat >> (4 + c % 2)) & 1 else -1) for c in range(4)]
            ext.append([s0 * rows[r] * cols[c] for r in range(4) for c in range(4)])
    d = np.ascontiguousarray(np.concatenate(blocks + [np.array(ext)]), np.int32)
    out = np.full(len(d), -1, np.int32)
    hip = api.Vp8Hip(16, 16)
    try:
        rc = hip.lib.vp8hip_debug_weight_mfma_rows(hip.h, C.c_void_p(d.ctypes.data), len(d), C.c_void_p(out.ctypes.data))
    finally:
        hip.close()
    assert rc == 0
    lib = Oracle.lib()
    exp = np.array([lib.vp8o_weight(row) for row in d], np.int32)
    bad = np.nonzero(out != exp)[0]
    assert bad.size == 0, (bad.size, bad[:5], d[bad[:2]], out[bad[:5]], exp[bad[:5]])


if __name__ == "__main__":
    assert os.environ.get("VP8HIP_S1_SPLIT") == "0", "run by the tests above, which force the loop form"
    found = 0
    for W, H in SHAPES:
        for way, which in (("batch of 4", None), ("batch of 1", ONE)):
            extremes = [] if which is None else None
            bad = _differences(W, H, which, extremes)
            print(_line(W, H, way) + str(bad), flush=True)
            found += len(bad)
            for level, ebad, (ext, wrap, far) in extremes or []:
                print(_extreme_line(W, H, level) + f"{ebad}; reach: {ext} extreme parent components, {wrap} blocks whose candidates pass int16, "
                      f"{far} vectors out beyond the frame", flush=True)
                found += len(ebad)
    sys.exit(1 if found else 0)
