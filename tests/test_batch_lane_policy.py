"""Which chain stream (lane) a new batch takes: the rule of vp8oclenc_amd/csrc/batch_lanes.h as host code
(scripts/native/batch_lane_policy.cpp), for 1..16 batches on L = 1..8 lanes with creations and destructions in random order.

What is asserted, and why not more.  A batch stays on its lane for life (moving it would mean re-ordering work another host thread
is enqueueing), so destructions can empty two lanes of four while the others keep three batches each, and no rule for the NEXT
creation can bring those loads within one of each other.  What a rule can promise, and this one does:
  * a creation takes a lane with the fewest batches, the lowest-numbered of them;
  * so the spread (most - fewest batches on a lane) after a creation is at most one wherever it was at most one before it, and
    never larger than before it -- in particular at most one, always, while nothing has been destroyed (batch i on lane i mod L),
    and again as soon as creations have refilled what destructions took;
  * the lane count is min(hardware queues, 8), at least 1.
No GPU."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("lanes") / "batch_lane_policy")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vp8oclenc_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "native", "batch_lane_policy.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=300)

    def run(commands):
        r = subprocess.run([exe], input="\n".join(commands) + "\n", check=True, capture_output=True, text=True, timeout=60)
        out = []
        for line in r.stdout.splitlines():
            w = line.split()
            out.append(int(w[1]) if w[0] == "lanes" else (int(w[1]), [int(x) for x in w[3:]]))
        assert len(out) == len(commands)
        return out
    return run


def test_the_lane_count_is_the_queue_count_up_to_eight(policy):
    got = policy([f"q {q}" for q in (-3, 0, 1, 2, 3, 4, 7, 8, 9, 16, 32)])
    assert got == [1, 1, 1, 2, 3, 4, 7, 8, 8, 8, 8]


@pytest.mark.parametrize("L", range(1, 9))
def test_without_destructions_batch_i_takes_lane_i_mod_l(policy, L):
    out = policy([f"q {L}"] + [f"c {i}" for i in range(16)])
    assert out[0] == L
    for i, (lane, loads) in enumerate(out[1:]):
        assert lane == i % L
        assert len(loads) == L and sum(loads) == i + 1
        assert max(loads) - min(loads) <= 1


def test_creations_and_destructions_in_random_order(policy):
    rng = random.Random(20240607)
    commands, model = [], []       # model: what the rule must do, restated here
    for L in range(1, 9):
        for nmax in range(1, 17):
            commands.append(f"q {L}")
            model.append(("q", L))
            alive, next_id = [], 0
            for _ in range(40):
                if alive and (len(alive) == nmax or rng.random() < 0.45):
                    b = alive.pop(rng.randrange(len(alive)))
                    commands.append(f"d {b}")
                    model.append(("d", b))
                else:
                    alive.append(next_id)
                    commands.append(f"c {next_id}")
                    model.append(("c", next_id))
                    next_id += 1
    out = policy(commands)
    loads, lane_of, balanced_runs = [], {}, 0
    for (op, arg), got in zip(model, out):
        if op == "q":
            assert got == arg
            loads, lane_of = [0] * arg, {}
            continue
        lane, reported = got
        spread_before = max(loads) - min(loads)
        if op == "c":
            assert loads[lane] == min(loads), "a creation takes a lane with the fewest batches"
            assert lane == loads.index(min(loads)), "... the lowest-numbered of them"
            loads[lane] += 1
            lane_of[arg] = lane
            spread = max(loads) - min(loads)
            assert spread <= max(1, spread_before)
            if spread_before <= 1:
                assert spread <= 1, "lane loads differ by at most one after a creation that found them so"
                balanced_runs += 1
        else:
            assert lane == lane_of.pop(arg), "a batch leaves the lane it was given"
            loads[lane] -= 1
        assert reported == loads
        assert min(loads) >= 0 and sum(loads) == len(lane_of)
    assert balanced_runs > 500      # (the sequences do visit the balanced case, not only the aftermath of destructions)
