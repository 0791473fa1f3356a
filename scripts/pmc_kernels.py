#!/usr/bin/env python3
"""Hardware counters of chosen kernels over one command: one rocprofv3 --pmc pass per counter set (a pass of its own each, no tracing
beside it), per kernel the launches, the mean per launch and the total of every counter, then the ratios a reader of an LDS question wants.

    python scripts/pmc_kernels.py --regex "k_search1_plr_b|k_search2_bs|k_mb_p|k_loop_filter3_b" \
        --set "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_INSTS_LDS" \
        --set "SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU" \
        --set "SQ_WAIT_INST_LDS SQ_WAIT_INST_ANY" \
        --out lds.txt -- python bench.py --gpus 1 --steps 20 --warmup 5

The command is started fresh under the profiler for every set; this program never opens the GPU itself.  A pass that fails or runs past
--timeout ends the whole run: nothing more is started after it."""
import argparse
import collections
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile


def one_pass(counters, regex, cmd, timeout):
    d = tempfile.mkdtemp(prefix="pmc_kernels_")
    try:
        full = ["rocprofv3", "--pmc"] + counters + ["--kernel-include-regex", regex, "-d", d, "-o", "p", "--output-format", "csv", "--"] + cmd
        r = subprocess.run(full, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=timeout)
        if r.returncode != 0:
            raise SystemExit("pmc_kernels: rc %d from the pass with %s\n%s" % (r.returncode, " ".join(counters), r.stderr[-2000:]))
        t = collections.defaultdict(list)
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                m = re.search(r"(k_[A-Za-z0-9_]+)", row["Kernel_Name"])
                t[(m.group(1) if m else row["Kernel_Name"][:40], row["Counter_Name"])].append(float(row["Counter_Value"]))
        return t
    finally:
        shutil.rmtree(d, ignore_errors=True)


RATIOS = [("LDS conflict share", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"),
          ("LDS array cycles per LDS instruction", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_LDS"),
          # (SQ_ACTIVE_INST_*, SQ_WAIT_* and SQ_WAVE_CYCLES count quad-cycles, summed over the four SIMDs of a CU: one unit per SIMD = one cycle of
          # the CU's four SIMDs side by side, which is what the CU's one LDS array is set against)
          ("LDS array cycles / VALU active quad-cycles", "SQ_LDS_IDX_ACTIVE", "SQ_ACTIVE_INST_VALU"),
          ("VALU active / wave cycles", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES"),
          ("waiting on LDS / waiting on anything", "SQ_WAIT_INST_LDS", "SQ_WAIT_INST_ANY"),
          ("waiting on LDS / wave cycles", "SQ_WAIT_INST_LDS", "SQ_WAVE_CYCLES")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--regex", required=True, help="kernels to count (rocprofv3 --kernel-include-regex)")
    ap.add_argument("--set", action="append", required=True, help="one pass: counter names separated by blanks (repeat for more passes)")
    ap.add_argument("--out", default=None, help="also write the table here")
    ap.add_argument("--label", default="", help="a line to head the table with")
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds one pass may take")
    ap.add_argument("cmd", nargs=argparse.REMAINDER, help="-- the command")
    a = ap.parse_args()
    cmd = a.cmd[1:] if a.cmd[:1] == ["--"] else a.cmd
    if not cmd:
        ap.error("no command after --")
    total = {}
    lines = [a.label] if a.label else []
    lines.append("command: " + " ".join(cmd))
    for s in a.set:
        t = one_pass(s.split(), a.regex, cmd, a.timeout)
        if not t:
            raise SystemExit("pmc_kernels: no counters came back for: " + s)
        for (k, c), v in sorted(t.items()):
            total[(k, c)] = sum(v)
            lines.append("%-20s %-24s %6d launches  %16.0f per launch  %18.0f total" % (k, c, len(v), sum(v) / len(v), sum(v)))
    for k in sorted({k for k, _ in total}):
        for name, num, den in RATIOS:
            if total.get((k, den)):
                lines.append("%-20s %-40s %.3f" % (k, name, total.get((k, num), 0.0) / total[(k, den)]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
