"""The references of tests/test_gpu_bool_coder.py, pinned to each other without a GPU: the oracle's serial boolean coder (the code the
reference's golden vectors vouch for) == its Python restatement == the exact big-number model, on every string family the device
is driven with; a decoder reads every bit back; and every constructed string meets, by the model alone, the condition it exists
for -- which lane, wave and step of k_ent_finish its propagate words, generating word and high halves fall into."""
import numpy as np
import pytest

import bool_coder_ref as R
from oracle_lib import oracle_bool_code
from vp8_parse import BoolDecoder
from vp8oclenc_amd import api

LADDERS = [(name, carried) for name in R.PLACEMENTS for carried in (True, False)]
LADDER_IDS = [f"{n}-{'carried' if c else 'standing'}" for n, c in LADDERS]


def three_ways(bools):
    m = R.Model(bools)
    ref = oracle_bool_code(bools)
    assert len(ref) == m.nbytes
    assert R.serial_encode(bools) == ref, "Python serial coder != oracle coder"
    assert m.bytes_from_value() == ref, "big number != oracle coder"
    assert m.bytes_from_words() == ref, "carry-resolved words != oracle coder"
    assert m.value_from_acc() == m.value and m.carry_out == 0
    assert max(m.t, default=0) < 1 << 33
    dec = BoolDecoder(ref)
    lst = np.asarray(bools).tolist()
    got = [dec.read(e & 255) for e in lst]
    assert got == [e >> 8 for e in lst], "the decoder does not read the bools back"
    return m


def word_at(m, d):
    return m.nw - 1 - d


@pytest.mark.parametrize("name,carried", LADDERS, ids=LADDER_IDS)
def test_ladder_three_ways_and_its_placement(name, carried):
    b = R.placement(name, carried)
    m = three_ways(b)
    assert m.t == R.model_of_placement(name, carried).t
    first = m.bytes_from_words()[:4]
    assert first == (b"\x80\x00\x00\x00" if carried else b"\x7f\xff\xff\xff")
    if name.startswith("lane63"):
        d = m.d(1)
        assert R.lane(d) == 63 and R.step(d) == 0 and (R.wave(d) == 15) == (name == "lane63_wave15") and R.wave(d) != 0
        assert not m.propagate(0) and m.t[0] == 0x7fffffff          # the word above takes the carry in and hands none on
        if carried:
            assert m.generate(1) and m.cin[0] == 1 and m.runs() == []
        else:
            assert m.propagate(1) and not m.generate(1) and m.cin[1] == 0 and m.cin[0] == 0 and m.runs() == [(d, d)]
        return
    runs = m.runs()
    assert len(runs) == 1, "a second run of propagate words would blur what the case shows"
    lo, hi = runs[0]
    assert lo == R.PLACEMENTS[name][1] and lo >= 1
    below, above = word_at(m, lo - 1), word_at(m, hi + 1)
    assert not m.propagate(above)
    for d in range(lo, hi + 1):
        assert m.cin[word_at(m, d)] == (1 if carried else 0)
    if carried:
        assert m.generate(below) and m.cin[above] == 1 and (above == 0 or m.cin[above - 1] == 0)     # the word above the run absorbs it
    else:
        assert not m.generate(below) and m.cin[above] == 0
    assert sum(m.generate(j) for j in range(m.nw)) == (1 if carried else 0)
    n = hi - lo + 1
    if name == "inside_wave":
        assert n >= 4 and R.step(lo) == R.step(hi) and R.wave(lo) == R.wave(hi) == R.wave(lo - 1) and R.lane(lo) >= 1
    elif name == "wave_seam":
        assert n < 64 and R.step(lo) == R.step(hi) and R.wave(hi) == R.wave(lo) + 1 and R.lane(lo) > R.lane(hi)
    elif name == "whole_wave":
        assert R.step(lo - 1) == R.step(hi) and R.wave(hi) - R.wave(lo) >= 2      # the waves between are all propagate words: Pw
    elif name == "step_seam":
        assert R.step(lo - 1) == R.step(lo) == 0 and R.step(hi) == 1 and n < 64
    elif name == "whole_step":
        assert n >= 1088 and R.step(lo - 1) == 0 and lo <= 1024 and hi >= 2048      # all sixteen waves of step 1, C in and C out
        assert all(m.propagate(word_at(m, d)) for d in range(1024, 2048))
    else:
        raise AssertionError(name)


def test_the_closers_without_a_tail_as_the_issue_states_them():
    """5 000 cycles: 15 002 bools, 4 377 bytes; (128, 1) leaves 1 091 propagate words with the generating word directly below and the
    output 80 00 00 00 ..; (128, 0) leaves 1 093 and no generating word, 7f ff ff ff .."""
    for carried, words, first in ((True, 1091, b"\x80\x00\x00\x00"), (False, 1093, b"\x7f\xff\xff\xff")):
        b = R.ladder_head(5000, carried)
        m = R.Model(b)
        assert len(b) == 15002 and m.nbytes == 4377
        (lo, hi), = m.runs()
        assert hi - lo + 1 == words
        assert m.generate(word_at(m, lo - 1)) == carried
        assert oracle_bool_code(b)[:4] == first == m.bytes_from_value()[:4]


def test_the_standing_tail_is_found_by_search_and_holds_for_every_ladder():
    seed = R.tail_seed(False)
    for n in (0, 1, 9, 40, 700):
        m = R.Model(np.concatenate([R.ladder_head(n, False), R.random_bools(seed, 300)]))
        assert m.bytes_from_words()[0] == 0x7f and not any(m.generate(j) for j in range(m.nw))
        if n >= 9:      # (with fewer cycles the tail's bits show in the first four bytes)
            m = R.Model(np.concatenate([R.ladder_head(n, True), R.random_bools(R.tail_seed(True), 300)]))
            assert m.bytes_from_words()[:4] == b"\x80\x00\x00\x00" and sum(m.generate(j) for j in range(m.nw)) == 1


@pytest.mark.parametrize("family", R.FAMILIES)
def test_seam_strings_three_ways(family):
    for b in R.seam_strings(family):
        three_ways(b)


def test_seam_strings_cover_the_sizes_and_the_straddling_adds():
    models = [R.Model(b) for f in R.FAMILIES for b in R.seam_strings(f)]
    assert {m.nbytes % 4 for m in models} == {0, 1, 2, 3}
    short = [m for m in models if m.w_end < 24]
    assert short and all(m.nbytes == 4 for m in short) and any(m.n > 0 and m.adds for m in short)
    assert any(m.n == 0 and m.nbytes == 4 and m.value == 0 for m in models)
    assert any((w & 31) > 24 for m in models for w, _ in m.adds)            # a split across two words
    assert any(m.n >= 2 * 8 * 256 + 1 for m in models)                       # more than two super-chunks of eight chunks
    for name, parts in (x for f in R.FAMILIES for x in R.seam_partitions(f)):
        assert len(parts) in (2, 3, 8)
    assert sum(len(b) for b in max((p for _, p in R.seam_partitions("uniform")), key=lambda p: sum(map(len, p)))) <= 102400


def test_dense_adds_three_ways_and_their_high_halves():
    """Largest high half of an accumulator seen: 126, in the string of (1, 1) alone (4 065 adds into one word, 127 of them at each of
    the seven bit positions whose split reaches into the next word); 63 with (255, 0) in turn; 9 in the random dense string (100 000
    bools, seven tenths of them (1, 1) or (255, 0), up to 87 adds into a word).  So t < 2^32 + 127: "tiny" holds, with room."""
    b = R.dense_string()
    m = three_ways(b)
    d = R.dense_condition(m)
    assert d is not None and d >= 1024 and R.lane(d) == 0 and R.wave(d) == 0 and m.high[word_at(m, d) + 1] != 0
    assert max(m.t) < 1 << 33
    assert max(m.high) >= 4 and max(m.adds_per_word) >= 64
    print("dense: high", max(m.high), "adds per word", max(m.adds_per_word), "t max", hex(max(m.t)))
    for kind in ("ones", "mixed"):
        p = three_ways(R.pure_dense(kind))
        assert max(p.t) < 1 << 33
        print(kind, "high", max(p.high), "adds per word", max(p.adds_per_word), "bytes", p.nbytes)
    assert max(R.Model(R.pure_dense("ones")).adds_per_word) >= 32 * 127 and max(R.Model(R.pure_dense("ones")).high) >= 100


def test_the_tap_is_declared_exported_and_bound():
    assert "vp8hip_debug_bool_code" in api.ABI_SYMBOLS and hasattr(api.load_library(), "vp8hip_debug_bool_code")
    assert callable(api.Vp8Hip.debug_bool_code)
