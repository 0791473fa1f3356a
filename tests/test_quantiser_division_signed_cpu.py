"""tdiv on the SIGNED numerator (kernels_mb.hip): C's truncating x / q as v_mul_hi_i32(x, M8) - (x >> 31) with M8 = (2^24 / q + 1) << 8, three
instructions where the magnitude through v_mul_hi_u32 and its sign put back were six.  The rule restated in numpy, not the device code (that is
held by test_gpu_quantiser_space.py and test_gpu_mb_small.py):

  * exact for every |x| < 2^15 and every 3 <= q < 512, exhaustively: v_mul_hi_i32 is floor(x * M / 2^24), which for x < 0 is one below
    -floor(|x| / q) as long as |x| * M is no multiple of 2^24, and the sign (x >> 31 = -1) subtracted puts the one back;
  * M8 is a positive int32 for those q;
  * q = 2 is OUTSIDE the rule, and no other multiplier mends it: its M8 is 2^31 + 256, which is negative as the signed operand the instruction
    takes, and x = 1 (quotient 0) wants a multiplier below 2^32 / 1 with a zero high half, i.e. m >= 0, while x = 2 (quotient 1) wants
    2m >= 2^32, i.e. m >= 2^31: no int32 is both.  (The unsigned rule of test_quantiser_space_cpu.py covers q = 2; the signed one cannot.)
  * and the kernel never divides by 2 or 3: a scan of the step tables over all 128 indices with every index delta of +-15 -- luma and chroma
    first order, the derived second-order steps, the chroma DC clamp -- finds steps 4 .. 440 and, besides them, only the forced luma DC step
    1 of an unsplit macroblock, which the kernel passes through without dividing (mb_dc_div)."""
import numpy as np

from vp8_decode import AC_Q, DC_Q


def m8(q):
    return ((1 << 24) // q + 1) << 8


def tdiv(x, q):
    """the three instructions, on int64 stand-ins of the 32-bit registers: v_mul_hi_i32, v_ashrrev_i32 31 (or its logical twin added), v_sub"""
    m = np.int64(m8(q))
    assert m < 1 << 31
    return ((x * m) >> np.int64(32)) - (x >> np.int64(31))


X = np.arange(-(1 << 15) + 1, 1 << 15, dtype=np.int64)          # every |x| < 2^15


def c_div(x, q):
    return np.sign(x) * (np.abs(x) // q)                         # C: toward zero


def test_the_signed_rule_is_c_division_for_every_numerator_and_every_quantiser_from_3():
    for q in range(3, 512):
        assert m8(q) < 1 << 31, q
        got = tdiv(X, q)
        assert np.array_equal(got, c_div(X, q)), (q, X[np.nonzero(got != c_div(X, q))[0][:4]])
        # what makes it exact: no |x| * M is a multiple of 2^24
        assert not ((np.abs(X[X != 0]) * np.int64(m8(q) >> 8)) % (1 << 24) == 0).any(), q


def test_quantiser_2_is_outside_the_signed_rule_and_why():
    assert m8(2) == (1 << 31) + 256                              # does not fit a positive int32
    # as the signed operand it would be taken for: wrong everywhere
    m = np.int64(m8(2) - (1 << 32))
    got = ((X * m) >> np.int64(32)) - (X >> np.int64(31))
    assert (got != c_div(X, 2))[X != 0].all()
    # and no int32 multiplier serves x = 1 and x = 2 together (high half of 1 * m is 0 iff 0 <= m; of 2 * m is 1 iff 2^31 <= m < 2^32)
    for mm in (0, 1, (1 << 31) - 1, -(1 << 31), -1):
        assert not ((1 * mm) >> 32 == 0 and (2 * mm) >> 32 == 1)


def qi(v):
    return min(max(v, 0), 127)


def test_the_forced_luma_dc_is_the_only_quantiser_below_4():
    steps = set()
    for i in range(128):
        steps.add(AC_Q[i])                                       # luma AC: k_ac_q[i]
        for d in range(-15, 16):
            steps.add(DC_Q[qi(i + d)])                           # luma DC of a split macroblock
            steps.add(min(DC_Q[qi(i + d)], 132))                 # chroma DC
            steps.add(AC_Q[qi(i + d)])                           # chroma AC
            steps.add(DC_Q[qi(i + d)] * 2)                       # y2dc
            steps.add(max(31 * AC_Q[qi(i + d)] // 20, 8))        # y2ac
    assert min(steps) == 4 and max(steps) == 440, (min(steps), max(steps))
    assert all(3 <= q < 512 for q in steps)
    # the one other divisor: dc_q = 1 where parts == 0 (GPU_kernels.cl:1394-1408), passed through, never multiplied
    assert 1 not in steps
