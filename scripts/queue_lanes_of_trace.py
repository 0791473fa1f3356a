#!/usr/bin/env python3
"""Which hardware queue did every batch chain of a rocprofv3 --kernel-trace CSV run on, and how busy was each queue?

    python scripts/queue_lanes_of_trace.py kt_kernel_trace.csv [nlf] [nbatches]

The window is that of scripts/concurrency_of_trace.py: the last `nlf` loop-filter launches (default 160).  A chain is a batch's
sequence of launches; it is recognised by its k_loop_filter*_b launches, one per batch and step.  The trace's Queue_Id is the
hardware queue, Stream_Id (where the profiler writes one) the HIP stream: two batches that share a lane (vp8hip_batch_lane) show as
one stream with twice the launches, so the chains of a stream or queue are its loop-filter launches over the launches of one chain
(all of them over `nbatches`, default 8).  Three tables: chains per queue, the share of the window every queue has a kernel
running, and the share of the window with 0, 1, 2, ... kernels running."""
import collections
import csv
import re
import sys


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    nlf = int(sys.argv[2]) if len(sys.argv) > 2 else 160
    nbatches = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    ev = []
    for r in rows:
        m = re.search(r"(k_[a-z0-9_]+)", r["Kernel_Name"])
        name = m.group(1) if m else r["Kernel_Name"][:16]
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r.get("Queue_Id", "?"), r.get("Stream_Id", "-")))
    ev.sort()
    lf = [e for e in ev if e[2].startswith("k_loop_filter")]
    if not lf:
        raise SystemExit("no loop-filter launches in the trace")
    t0, t1 = lf[-min(nlf, len(lf))][0], lf[-1][1]
    sel = [e for e in ev if e[0] >= t0 and e[1] <= t1]
    win = t1 - t0
    print("window %.1f ms, %d kernels, %d hardware queues, %d streams" % (win / 1e6, len(sel), len({e[3] for e in sel}), len({e[4] for e in sel})))

    # ---- chains per queue ----------------------------------------------------------------------------------------------
    chain_lf = [e for e in sel if re.match(r"k_loop_filter\w*_b", e[2])]
    per_chain = max(1.0, len(chain_lf) / nbatches)
    by_queue = collections.defaultdict(collections.Counter)
    for e in chain_lf:
        by_queue[e[3]][e[4]] += 1
    print("batch chains per hardware queue (%d batched loop-filter launches, %.1f per chain):" % (len(chain_lf), per_chain))
    shares = []
    for q in sorted({e[3] for e in sel}, key=lambda s: (len(s), s)):
        streams = by_queue.get(q, {})
        n = sum(streams.values())
        shares.append(n / per_chain)
        detail = ", ".join("stream %s: %d launches = %.1f chains" % (s, c, c / per_chain) for s, c in sorted(streams.items(), key=lambda kv: (len(kv[0]), kv[0])))
        print("  queue %-4s %4.1f chains   %s" % (q, n / per_chain, detail or "(no chain)"))
    with_chain = [s for s in shares if s > 0.25]
    print("  queues with a chain: %d; most on one queue %.1f, fewest %.1f" % (len(with_chain), max(with_chain, default=0), min(with_chain, default=0)))

    # ---- busy share per queue ------------------------------------------------------------------------------------------
    print("share of the window with a kernel running, per hardware queue:")
    for q in sorted({e[3] for e in sel}, key=lambda s: (len(s), s)):
        iv = sorted((e[0], e[1]) for e in sel if e[3] == q)
        busy, end = 0, t0
        for a, b in iv:      # (a queue is in order, but its kernels may still overlap where no barrier stands between them: union)
            if b > end:
                busy += b - max(a, end)
                end = b
        print("  queue %-4s %.3f   (%d kernels)" % (q, busy / win, len(iv)))

    # ---- kernels at once -----------------------------------------------------------------------------------------------
    pts = []
    for e in sel:
        pts.append((e[0], 1))
        pts.append((e[1], -1))
    pts.sort()
    cur, last, hist = 0, t0, collections.Counter()
    for t, d in pts:
        hist[cur] += t - last
        last = t
        cur += d
    tot = sum(hist.values())
    print("kernels running at once (% of time):", {k: round(100 * v / tot, 1) for k, v in sorted(hist.items())})
    print("  %.2f running on average" % (sum(k * v for k, v in hist.items()) / tot))
    busy, cnt = collections.Counter(), collections.Counter()
    for e in sel:
        busy[e[2]] += e[1] - e[0]
        cnt[e[2]] += 1
    for k, v in busy.most_common(10):
        print("  %-24s %5d launches  avg %7.1f us   %.2f running on average" % (k, cnt[k], v / cnt[k] / 1e3, v / win))


if __name__ == "__main__":
    main()
