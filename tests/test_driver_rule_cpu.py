"""The driver's refusal table (vp8oclenc_amd/csrc/driver_settings.h) against the refusals of the native frame loop restated setter by
setter, each as the chain of ifs its entry point was written as -- two forms of independent shape -- over the WHOLE space of the facts a
refusal reads: every boolean both ways, every small integer through its off value and an on value (the deinterlacer through both modes),
for every feature, asked for and dropped.  Every verdict must match.  And operator== over what the members of a batch must share: a
candidate that differs from another in one shared field may not share its batch, one that differs in any other field may.  The table
runs in a stand-alone program (scripts/native/driver_rule_check.cpp) under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include")]
SHARED = ["qi_min", "qi_max", "num_partitions", "loop_filter_type", "in_width", "in_height", "scale_filter", "check_ssim", "denoise", "deinterlace", "field",
          "format", "colour", "transfer", "peak", "analysis", "seg_mode", "seg_strength"]
FIELDS = SHARED + ["device_params", "overlap_filter", "scene_detect", "quality_stats", "ssim_target", "scheduled_altref", "window", "canvas", "arf", "tl_layers", "tl_next",
                   "tl_flags", "ir_period", "in_batch", "hidden_shapes_refs", "shard", "overlays"]
# the facts a refusal reads and the values each goes through; every other field stands at BASE's value
SPACE = dict(device_params=(0, 1), overlap_filter=(0, 1), scene_detect=(0, 1), quality_stats=(0, 1), ssim_target=(0, 1), scheduled_altref=(0, 1), window=(0, 1),
             in_batch=(0, 1), hidden_shapes_refs=(0, 1), shard=(0, 1), analysis=(0, 1), denoise=(0, 2), format=(0, 1), deinterlace=(0, 1, 2), tl_layers=(1, 3),
             tl_next=(1, 3), arf=(0, 4), ir_period=(0, 8), canvas=(0, 2))
BASE = dict(dict.fromkeys(FIELDS, 0), qi_max=9, num_partitions=1, check_ssim=1, device_params=1, tl_layers=1, tl_next=1)
OK, ARG, STATE = ord("."), ord("A"), ord("S")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("driver_rule") / "driver_rule_check")
    subprocess.run(SAN + [os.path.join(ROOT, "scripts", "native", "driver_rule_check.cpp"), "-o", exe], check=True, timeout=600)

    def run(text, *args):
        r = subprocess.run([exe, *args], input=text, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stdout
    run.exe = exe
    return run


def chain(n, *clauses):
    """a chain of `if (clause) return code;` that ends in `return VP8HIP_OK;`, over n candidates at once"""
    out = np.full(n, OK, np.uint8)
    open_ = np.ones(n, bool)
    for clause, code in clauses:
        out[open_ & clause] = code
        open_ &= ~clause
    return out


# ---- the entry points' refusals, each as it was written (s: the facts, arrays of one value per candidate) -----------------------------
def set_arf(s, strength):
    return chain(s.n,
                 (strength & (~s.device_params | s.overlap_filter | (s.format != 0) | s.window | (s.deinterlace != 0) | (s.denoise != 0) | s.analysis), ARG),
                 (s.in_batch | (strength & ((s.canvas != 0) | (s.tl_layers > 1) | (s.tl_next > 1))), STATE))


def set_temporal_layers(s, layers):
    more = np.bool_(layers > 1)
    return chain(s.n,
                 (more & (~s.device_params | s.overlap_filter | s.scheduled_altref), ARG),
                 (more & (s.in_batch | (s.arf != 0) | s.shard), STATE))


def set_intra_refresh(s, period):
    on = np.bool_(period != 0)
    return chain(s.n,
                 (on & (~s.device_params | s.ssim_target), ARG),
                 (on & (s.in_batch | s.shard), STATE))


def set_canvas(s, n):
    return chain(s.n,
                 (~s.device_params, ARG),
                 (np.bool_(n != 0) & (s.in_batch | (s.arf != 0)), STATE))


def intake_setter(s):
    """vp8drv_set_denoise, _deinterlace, _source_format, _source_colour, _source_transfer, _source_window, _source_orientation, _analysis"""
    return chain(s.n, (~s.device_params, ARG), (s.in_batch, STATE))


def batch_member(s):
    return chain(s.n,
                 (~s.device_params | s.overlap_filter | s.scene_detect | (s.arf != 0) | (s.canvas != 0) | s.hidden_shapes_refs |
                  (s.tl_layers > 1) | (s.tl_next > 1) | (s.ir_period != 0), ARG))


def batch_scan(s):
    return chain(s.n, ((s.denoise != 0) | (s.deinterlace == 2) | s.analysis | s.quality_stats, STATE))


def test_the_table_is_the_entry_points_refusals_over_the_whole_space(program):
    names = list(SPACE)
    grids = np.meshgrid(*[np.array(SPACE[k], np.uint8) for k in names], indexing="ij")
    value = {k: g.ravel() for k, g in zip(names, grids)}
    n = value[names[0]].size
    assert n == 3 * 2 ** 18
    booleans = {k for k in names if SPACE[k] == (0, 1)}
    s = types.SimpleNamespace(n=n, **{k: (v != 0) if k in booleans else v.astype(np.int32) for k, v in value.items()})
    yes, no = np.bool_(True), np.bool_(False)
    same = [intake_setter(s), batch_member(s), batch_scan(s)]
    want = np.stack([set_arf(s, yes), set_temporal_layers(s, 3), set_intra_refresh(s, 8), set_canvas(s, 2)] + same +
                    [set_arf(s, no), set_temporal_layers(s, 1), set_intra_refresh(s, 0), set_canvas(s, 0)] + same, axis=1)
    # the candidates as text: every value here is one digit
    text = np.full((n, 2 * len(FIELDS) + 4), ord(" "), np.uint8)
    for k, name in enumerate(FIELDS):
        text[:, 2 * k] = ord("0") + (value[name] if name in value else BASE[name])
    text[:, -4:] = np.frombuffer(b"* 1\n", np.uint8)
    got = np.frombuffer(program(text.tobytes()), np.uint8)
    assert got.size == n * 15
    got = got.reshape(n, 15)
    assert (got[:, 14] == ord("\n")).all()
    bad = np.argwhere(got[:, :14] != want)
    if len(bad):
        i, f = bad[0]
        what = (["ARF", "LAYERS", "INTRA_REFRESH", "CANVAS", "INTAKE_SETTER", "BATCH_MEMBER", "SCAN"] * 2)[f] + (" asked for" if f < 7 else " dropped")
        raise AssertionError(f"{len(bad)} verdicts differ; the first: {what} with {({k: int(v[i]) for k, v in value.items()})}: {chr(got[i, f])} for {chr(want[i, f])}")
    # every code occurs for every feature that has it, so no column is trivially right
    for f, codes in enumerate(("AS.", "AS.", "AS.", "AS.", "AS.", "A.", "S.")):
        assert set(np.unique(want[:, f])) == {ord(c) for c in codes}, f
    assert (want[:, 8] == OK).all() and (want[:, 9] == OK).all()      # one layer and period 0 are always accepted


def line(candidate, feature="*", on=1):
    return " ".join(str(int(candidate[k])) for k in FIELDS) + f" {feature} {on}\n"


def test_single_features_and_the_line_format(program):
    member = dict(BASE, in_batch=1)
    asks = [(BASE, "ARF", 1, "."), (member, "ARF", 1, "S"), (member, "ARF", 0, "S"), (member, "LAYERS", 0, "."), (dict(BASE, device_params=0), "CANVAS", 0, "A"),
            (dict(BASE, qi_max=127, peak=10000, in_width=16384, deinterlace=2), "SCAN", 1, "S"), (dict(BASE, arf=7), "BATCH_MEMBER", 1, "A")]
    out = program("".join(line(c, f, on) for c, f, on, _ in asks).encode()).decode().split()
    assert out == [w for *_, w in asks]
    for bad in ("1 2 3\n", line(BASE, "NOTHING"), line(BASE).replace("*", "")):
        r = subprocess.run([program.exe], input=bad.encode(), capture_output=True, timeout=60)
        assert r.returncode == 1 and b"no candidate" in r.stderr, bad


def test_members_agree_on_the_shared_fields_and_on_nothing_else(program):
    base = dict(BASE, qi_min=4, in_width=128, in_height=96, scale_filter=1, denoise=1, deinterlace=1, transfer=1, peak=1000, seg_mode=2, seg_strength=2)
    pairs, want = [line(base) + line(base)], ["same"]
    for k in FIELDS:
        for other in (base[k] + 1, 0 if base[k] else 1):
            if other == base[k] or (k in ("check_ssim", "analysis") and other > 1):      # (the two are booleans: 2 is 1)
                continue
            pairs.append(line(base) + line(dict(base, **{k: other})))
            want.append("differ" if k in SHARED else "same")
    got = program("".join(pairs).encode(), "agree").decode().split()
    assert got == want, [(p.splitlines()[1], g, w) for p, g, w in zip(pairs, got, want) if g != w][:3]
