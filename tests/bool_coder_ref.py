"""The boolean coder (RFC 6386 section 7.3; oracle/vp8_entropy_oracle.c put_bool / flush) three times over, and the bool strings
that drive the device's parallel coder (vp8oclenc_amd/csrc/kernels_ent.hip, part 2) where coefficient data never takes it:

  serial_encode   the serial coder, restated in plain Python;
  Model           the exact arithmetic the parallel coder is built on: a partition is the big number
                      sum_i add_i * 2^(8 * nbytes - 8 - W_i)      (add_i = split if bool i is 1, W_i = shifts before bool i)
                  plus what the device makes of it on the way: the 64-bit accumulator per 32 output bits (k_ent_encode), the
                  pre-carry words t[j] = low32(acc[j]) + (acc[j + 1] >> 32) and the carry into every word (k_ent_finish);
  ladder, ...     the constructions: carry ladders placed by search, random strings per probability family, dense adds.

A bool is probability | bit << 8 (the device's encoding); a string is a uint16 array.  Word j = 0 holds the partition's first four
bytes.  k_ent_finish walks a partition from its last word up, 1024 words per step, sixteen waves of 64 lanes: word j sits at
distance d = nw - 1 - j from the last word, in lane d % 64 of wave (d // 64) % 16 of step d // 1024.
"""
from __future__ import annotations

import functools

import numpy as np

M32 = 0xffffffff
LENGTHS = (0, 1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 20000)
FAMILIES = ("uniform", "extreme", "half", "zeros", "ones")


def pack(pairs) -> np.ndarray:
    return np.array([p | (b << 8) for p, b in pairs], np.uint16)


# ---- the serial coder ------------------------------------------------------------------------------------------------------------
def serial_encode(bools) -> bytes:
    out = bytearray()
    rng, bottom, bit_count = 255, 0, 24

    def carry():
        i = len(out) - 1
        while out[i] == 255:
            out[i] = 0
            i -= 1
        out[i] += 1

    for e in np.asarray(bools).tolist():
        split = 1 + (((rng - 1) * (e & 255)) >> 8)
        if e >> 8:
            bottom = (bottom + split) & M32
            rng -= split
        else:
            rng = split
        while rng < 128:
            rng <<= 1
            if bottom & 0x80000000:
                carry()
            bottom = (bottom << 1) & M32
            bit_count -= 1
            if bit_count == 0:
                out.append(bottom >> 24)
                bottom &= 0xffffff
                bit_count = 8
    c, v = bit_count, bottom
    if v & (1 << (32 - c)):
        carry()
    v = (v << (c & 7)) & M32
    for _ in range(c >> 3):
        v = (v << 8) & M32
    for _ in range(4):
        out.append(v >> 24)
        v = (v << 8) & M32
    return bytes(out)


# ---- the exact model -------------------------------------------------------------------------------------------------------------
def trace(bools, rng: int = 255):
    """The range recursion alone: ([(W_i, split_i) of the bools that are 1], shifts after the last bool, range after it)."""
    W, adds = 0, []
    for e in bools:
        split = 1 + (((rng - 1) * (e & 255)) >> 8)
        if e >> 8:
            adds.append((W, split))
            rng -= split
        else:
            rng = split
        if rng < 128:
            z = 8 - rng.bit_length()
            rng <<= z
            W += z
    return adds, W, rng


def _weighted_sum(adds, lo: int, hi: int):
    """sum of split << (W_last - W) over adds[lo:hi], W_last = W of adds[hi - 1]; halves combined, so that no step moves a long number
    by a short distance"""
    if hi - lo <= 32:
        last = adds[hi - 1][0]
        return sum(s << (last - w) for w, s in adds[lo:hi]), last
    mid = (lo + hi) // 2
    a, wa = _weighted_sum(adds, lo, mid)
    b, wb = _weighted_sum(adds, mid, hi)
    return (a << (wb - wa)) + b, wb


class Model:
    def __init__(self, bools):
        lst = np.asarray(bools).tolist()
        self.n = len(lst)
        adds, W, _ = trace(lst)
        self.adds, self.w_end = adds, W
        self.nbytes = ((W - 24) // 8 + 1 if W >= 24 else 0) + 4      # bytes emitted while coding + the flush's four
        self.nw = nw = (self.nbytes + 3) // 4
        # the big number
        if adds:
            v, last = _weighted_sum(adds, 0, len(adds))
            self.value = v << (8 * self.nbytes - 8 - last)
        else:
            self.value = 0
        # the device's accumulators: a split lies at stream bits W .. W + 7, in word W >> 5 and perhaps the next one
        acc = [0] * (nw + 1)
        per_word = [0] * (nw + 1)
        for w, s in adds:
            o, j = w & 31, w >> 5
            per_word[j] += 1
            if o <= 24:
                acc[j] += s << (24 - o)
            else:
                acc[j] += s >> (o - 24)
                acc[j + 1] += (s << (56 - o)) & M32
        assert acc[nw] == 0
        self.acc = acc[:nw]
        self.adds_per_word = per_word[:nw]
        self.high = [a >> 32 for a in self.acc]
        self.t = [(self.acc[j] & M32) + (self.high[j + 1] if j + 1 < nw else 0) for j in range(nw)]
        # the carries, serially from the last word up
        self.cin = [0] * nw
        words, c = [0] * nw, 0
        for j in range(nw - 1, -1, -1):
            self.cin[j] = c
            x = self.t[j] + c
            words[j] = x & M32
            c = x >> 32
        self.carry_out = c
        self.words = words

    # three ways to the same bytes
    def bytes_from_value(self) -> bytes:
        return self.value.to_bytes(self.nbytes, "big")

    def bytes_from_words(self) -> bytes:
        return b"".join(w.to_bytes(4, "big") for w in self.words)[:self.nbytes]

    def value_from_acc(self) -> int:
        v = 0
        for a in self.acc:
            v = (v << 32) + a
        return v >> (8 * (4 * self.nw - self.nbytes))

    # where k_ent_finish meets word j
    def d(self, j: int) -> int:
        return self.nw - 1 - j

    def propagate(self, j: int) -> bool:
        return (self.t[j] & M32) == M32

    def generate(self, j: int) -> bool:
        return (self.t[j] >> 32) != 0

    def runs(self):
        """maximal runs of propagate words as (d of the least significant word, d of the most significant one), longest first"""
        out, j = [], 0
        while j < self.nw:
            if self.propagate(j):
                k = j
                while k + 1 < self.nw and self.propagate(k + 1):
                    k += 1
                out.append((self.d(k), self.d(j)))
                j = k + 1
            else:
                j += 1
        return sorted(out, key=lambda r: r[0] - r[1])

    def longest_run(self):
        r = self.runs()
        return r[0] if r else None

    def carry_into_d(self, d: int) -> int:
        return self.cin[self.nw - 1 - d]


def lane(d: int) -> int:
    return d % 64


def wave(d: int) -> int:
    return (d // 64) % 16


def step(d: int) -> int:
    return d // 1024


# ---- strings ---------------------------------------------------------------------------------------------------------------------
def random_bools(seed: int, m: int, family: str = "uniform") -> np.ndarray:
    """m random bools.  uniform: probability 1..255; extreme: {1, 2, 254, 255}; half: 128; zeros / ones: uniform probabilities,
    95 % of the bits 0 / 1."""
    rng, rbit = (np.random.default_rng([seed, FAMILIES.index(family), k]) for k in (0, 1))   # (a longer string continues a shorter one)
    if family == "extreme":
        prob = np.array([1, 2, 254, 255])[rng.integers(0, 4, m)]
    elif family == "half":
        prob = np.full(m, 128)
    else:
        prob = rng.integers(1, 256, m)
    if family == "zeros":
        bit = rbit.random(m) < 0.05
    elif family == "ones":
        bit = rbit.random(m) < 0.95
    else:
        bit = rbit.integers(0, 2, m)
    return (prob.astype(np.uint16) | (bit.astype(np.uint16) << 8)).astype(np.uint16)


def dense_bools(seed: int, m: int, rich: float = 0.7) -> np.ndarray:
    """a share `rich` of (1, 1) and (255, 0) -- a bool of either kind takes one off the range, and (1, 1) adds, without a shift until
    the range reaches 127 -- among uniform random bools, which supply most of the shifts"""
    pick = np.random.default_rng([seed, 77]).random(m)
    b = random_bools(seed, m, "uniform")
    b[pick < rich] = 255
    b[pick < rich * 0.6] = 1 | (1 << 8)
    return b


def pure_dense(kind: str, m: int = 30000) -> np.ndarray:
    """ones: (1, 1) only -- 127 adds of 1 at every bit position, some four thousand into one word; mixed: (1, 1), (255, 0) in turn"""
    b = np.full(m, 1 | (1 << 8), np.uint16)
    if kind == "mixed":
        b[1::2] = 255
    return b


def ladder_head(n: int, carried: bool) -> np.ndarray:
    """(127, 1) leaves bottom = 01111111 and range 128: the interval straddles 1/2.  Each cycle (3, 0), (125, 1), (1, 1) adds seven
    ones and leaves it straddling.  The closer (128, 1) then carries through all of them; (128, 0) lets them stand."""
    return pack([(127, 1)] + n * [(3, 0), (125, 1), (1, 1)] + [(128, 1 if carried else 0)])


@functools.lru_cache(maxsize=None)
def tail_seed(carried: bool) -> int:
    """After (128, 1) the carry is settled.  After (128, 0) the interval still reaches across the boundary, and the bools that follow
    decide: the first seed whose random tail lets the ones stand (the state after the closer is the same for every n)."""
    if carried:
        return 1
    for seed in range(1, 4096):
        if Model(np.concatenate([ladder_head(12, False), random_bools(seed, 256)])).words[0] == 0x7fffffff:
            return seed
    raise ValueError("no seed below 4096 lets the run stand")


@functools.lru_cache(maxsize=None)
def _tail_shifts(n: int, carried: bool, mmax: int):
    head = ladder_head(n, carried)
    _, W, r = trace(head.tolist())
    tail = random_bools(tail_seed(carried), mmax)
    cum, Wt = [0], 0
    for e in tail.tolist():
        split = 1 + (((r - 1) * (e & 255)) >> 8)
        r = r - split if e >> 8 else split
        if r < 128:
            z = 8 - r.bit_length()
            r <<= z
            Wt += z
        cum.append(Wt)
    probe = Model(np.concatenate([head, tail[:256]]))
    return head, tail, W, cum, probe


@functools.lru_cache(maxsize=None)
def ladder(n: int, carried: bool, d: int, anchor: int = -1, mmax: int = 60000) -> np.ndarray:
    """The ladder of n cycles followed by as many random bools as put word `anchor` (-1: the least significant word of its run of
    propagate words) at distance d from the partition's last word: the tail moves the end of the partition, not the run."""
    head, tail, W, cum, probe = _tail_shifts(n, carried, mmax)
    if anchor < 0:
        anchor = probe.nw - 1 - probe.longest_run()[0]
    want_nw = d + 1 + anchor
    lo_m, hi_m = 0, mmax
    nw_of = lambda m: ((((W + cum[m] - 24) // 8 + 1 if W + cum[m] >= 24 else 0) + 4) + 3) // 4
    if not nw_of(0) <= want_nw <= nw_of(mmax):
        raise ValueError(f"ladder({n}, {carried}, {d}): {want_nw} words are outside {nw_of(0)}..{nw_of(mmax)}")
    while lo_m < hi_m:        # the first m with enough words (a bool adds at most seven bits: no count is stepped over)
        mid = (lo_m + hi_m) // 2
        if nw_of(mid) < want_nw:
            lo_m = mid + 1
        else:
            hi_m = mid
    return np.concatenate([head, tail[:lo_m]])


# The placements of the carry ladders: name -> (cycles, d, anchor word).  With seven bits a cycle a run is about 7 n / 32 words long;
# under the carrying closer the generating word is the word directly below the run, at d - 1.  With 9 to 13 cycles the ones end
# with word 1: word 0 is 0x7fffffff, word 1 generates (carrying closer) or is a lone propagate word (standing closer).
PLACEMENTS = {
    "inside_wave": (40, 5 * 64 + 20, -1),      # six words in lanes 20.. of wave 5
    "wave_seam": (40, 3 * 64 - 4, -1),         # ... from lane 60 of wave 2 into wave 3
    "whole_wave": (700, 2 * 64 - 10, -1),      # some 150 words: all of wave 2 and more
    "step_seam": (40, 1020, -1),               # from wave 15 of step 0 into step 1; the generating word in step 0
    "whole_step": (5000, 1000, -1),            # 1 091 words: all of step 1, a carry into it from step 0 and out of it into step 2
    "lane63": (10, 4 * 64 + 63, 1),            # word 1 at lane 63 of wave 4, the word above it no propagate word
    "lane63_wave15": (10, 1023, 1),            # ... of wave 15: the carry leaves the step
}


def placement(name: str, carried: bool) -> np.ndarray:
    n, d, anchor = PLACEMENTS[name]
    return ladder(n, carried, d, anchor)


@functools.lru_cache(maxsize=None)
def model_of_placement(name: str, carried: bool) -> Model:
    return Model(placement(name, carried))


def dense_condition(m: Model):
    """a word at lane 0 of wave 0 of a step other than the first whose neighbour below (lane 63 of wave 15 of the step before) has a
    non-zero high half: -> its d, or None"""
    for j in range(m.nw - 1):
        d = m.d(j)
        if d >= 1024 and d % 1024 == 0 and m.high[j + 1] != 0:
            return d
    return None


@functools.lru_cache(maxsize=None)
def dense_string() -> np.ndarray:
    """the first dense string (by seed) of 100 000 bools that meets dense_condition"""
    for seed in range(200, 264):
        b = dense_bools(seed, 100000)
        if dense_condition(Model(b)) is not None:
            return b
    raise ValueError("no seed in 200..263 meets the dense-add condition")


def seam_strings(family: str):
    """one random string per length of LENGTHS"""
    return [random_bools(1000 + i, n, family) for i, n in enumerate(LENGTHS)]


def seam_partitions(family: str):
    """(name, strings per partition) for P = 2, 3, 8: mixed lengths, alternating empty / full, all empty"""
    s = seam_strings(family)
    by = dict(zip(LENGTHS, s))
    e = by[0]
    return [
        ("P2", [by[257], by[2049]]),
        ("P2_empty_first", [e, by[4097]]),
        ("P3", [by[33], by[20000], by[511]]),
        ("P3_empty_middle", [by[256], e, by[1]]),
        ("P8", [by[n] for n in (2, 31, 32, 255, 512, 513, 2047, 4095)]),
        ("P8_alternating", [e, by[2048], e, by[4096], e, by[20000], e, by[1]]),
        ("P8_all_empty", [e] * 8),
        ("P3_all_empty", [e] * 3),
    ]
