"""The block-match metric in the form the search kernels run (weight_mfma, vp8hip_dev.h: the column pass as one
v_mfma_i32_32x32x32_i8 per wave, every lane on its own 4x4 block) against the CPU restatement.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import Oracle
from vp8oclenc_amd import api

pytestmark = pytest.mark.gpu


def test_block_match_metric_mfma_form_vs_oracle():
    """200k random difference blocks of every amplitude plus the extreme sign-pattern blocks that bound the int16 ranges.  Every
    lane of the tap carries a different block -- lanes 32-63 included, which read the other half of the block-diagonal A table --
    so a wrong row or half of the table shows up as a mismatch."""
    rng = np.random.default_rng(11)
    blocks = [rng.integers(-a, a + 1, size=(40000, 16)) for a in (1, 4, 32, 128, 255)]
    ext = []
    for s0 in (-255, 255):
        for pat in range(64):      # sign patterns over rows/columns drive every butterfly to its extreme
            rows = [(1 if (pat >> r) & 1 else -1) for r in range(4)]
            cols = [(1 if (pat >> (4 + c % 2)) & 1 else -1) for c in range(4)]
            ext.append([s0 * rows[r] * cols[c] for r in range(4) for c in range(4)])
    d = np.ascontiguousarray(np.concatenate(blocks + [np.array(ext)]), np.int32)
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
