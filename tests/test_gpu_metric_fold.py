"""The folded form of the block-match metric (weight_mfma, vp8hip_dev.h): the matrix instruction delivers, for rows 0 and 2 of the
column pass, the row butterfly itself -- s = R[0] + R[1] + R[2] + R[3], m = R[0] - R[1] - R[2] + R[3], c = R[1] - R[2], d = R[0] - R[3]
-- and the packed 16-bit steps behind it rest on |s|, |m| <= 32640 and |c|, |d| <= 16320.  Difference blocks that drive each of the
four to its bound, against the CPU restatement: d[r][c] = amplitude * (row sign r) * (column factor c), the row signs all 16 patterns
(one of them makes every R0[c], another every R2[c], extreme), the column factors all 81 patterns over {-1, 0, +1} (+ + + + for s,
+ - - + for m, 0 + - 0 for c, + 0 0 - for d, and every mixture).  test_gpu_metric_mfma.py's column signs have period 2 and reach
neither m nor d.  Run with `pytest -m gpu`."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle_lib import Oracle
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu


def _blocks():
    out = []
    for amp in (255, -255, 1, -1):
        for pat in range(16):
            rows = [1 if (pat >> r) & 1 else -1 for r in range(4)]
            for cols in itertools.product((-1, 0, 1), repeat=4):
                out.append([amp * rows[r] * cols[c] for r in range(4) for c in range(4)])
    return np.array(out, np.int32)


def test_the_folded_metric_on_blocks_that_drive_every_new_quantity_to_its_bound():
    """Every block twice, 32 blocks apart modulo 64: block i of the tap is lane i & 63 of its wave, so each block meets both halves of the
    block-diagonal A table (lanes 0-31 and 32-63)."""
    blocks = _blocks()
    assert len(blocks) == 5184 and len(blocks) % 64 == 0
    d = np.ascontiguousarray(np.concatenate([blocks, np.zeros((32, 16), np.int32), blocks]), np.int32)
    half = (np.arange(len(d)) & 63) >> 5
    assert np.all(half[:5184] != half[5184 + 32:])
    out = np.full(len(d), -1, np.int32)
    hip = api.Vp8Hip(16, 16)
    try:
        rc = hip.lib.vp8hip_debug_weight_mfma(hip.h, C.c_void_p(d.ctypes.data), len(d), C.c_void_p(out.ctypes.data))
    finally:
        hip.close()
    assert rc == 0
    lib = Oracle.lib()
    exp = np.array([lib.vp8o_weight(row) for row in d], np.int32)
    bad = np.nonzero(out != exp)[0]
    assert bad.size == 0, (bad.size, bad[:5], d[bad[:2]], out[bad[:5]], exp[bad[:5]])
