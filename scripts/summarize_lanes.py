#!/usr/bin/env python3
"""Where the two lanes of bench.py's timed region sit against each other, from a kernel trace.

  rocprofv3 --kernel-trace --stats -d DIR -- python3 bench.py --role worker --gpus 1 --steps K --warmup W ...
  python3 scripts/summarize_lanes.py DIR/**/*_kernel_trace.csv --steps K

A step of a lane is the chain  ph_tiny_prep_kernel, 2 x ph_tiny_pack_kernel, ph_tiny_table_mfma_kernel,
ph_search_kernel  on that lane's hardware queue (prep and the node-side pack are absent when the workspace kept them).
The timed steps are the last K search kernels of a plain run: nothing searches after them.  Printed, for those steps:

  ms_per_step        first start to last end of their kernels, over K (bench.py's figure, minus launch latency)
  table wait         for each table kernel: start minus the end of the previous search kernel on its queue (the
                     moment stream order lets it run), its duration, and how long before the end of the search
                     kernel running on the OTHER queue it started (as ms and as a share of that kernel's time)
  search + search    time during which two search kernels are resident together
  table + search     time during which a table kernel and a search kernel are resident together

Timestamps are the dispatch's: a kernel whose blocks wait for room on the CUs has started by this clock, which is why
the duration of every table kernel is printed beside its start (1.2 ms alone; longer when it is squeezed in)."""
import argparse
import csv
import statistics
import sys

SEARCH, TABLE = "ph_search_kernel", "ph_tiny_table"
CHAIN = ("ph_tiny_prep_kernel", "ph_tiny_pack_kernel", TABLE)


def read_trace(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            try:
                t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            except (KeyError, ValueError):
                continue
            rows.append({"name": name, "q": r.get("Queue_Id", "0"), "t0": t0, "t1": t1,
                         "lds": r.get("LDS_Block_Size", ""), "vgpr": r.get("VGPR_Count", "")})
    rows.sort(key=lambda r: r["t0"])
    return rows


def overlap(a, b):
    return max(0, min(a["t1"], b["t1"]) - max(a["t0"], b["t0"]))


def union_ms(spans):
    total, end = 0, None
    for t0, t1 in sorted(spans):
        if end is None or t0 > end:
            total += t1 - t0
            end = t1
        elif t1 > end:
            total += t1 - end
            end = t1
    return total / 1e6


def summarize(rows, steps):
    searches = [r for r in rows if SEARCH in r["name"]]
    if len(searches) < steps + 1:
        raise SystemExit("the trace holds %d search kernels, fewer than --steps + 1" % len(searches))
    timed = searches[-steps:]
    out = []
    per_step, members = [], []
    for s in timed:
        prev = [p for p in searches if p["q"] == s["q"] and p["t1"] <= s["t0"]]
        prev_end = prev[-1]["t1"] if prev else None
        chain = [r for r in rows if r["q"] == s["q"] and any(c in r["name"] for c in CHAIN)
                 and r["t0"] < s["t0"] and (prev_end is None or r["t0"] >= prev_end)]
        table = [r for r in chain if TABLE in r["name"]]
        members += chain + [s]
        per_step.append((s, prev_end, chain, table[-1] if table else None))
    first, last = min(r["t0"] for r in members), max(r["t1"] for r in members)
    out.append("timed steps: %d, queues %s" % (steps, sorted({s["q"] for s in timed})))
    out.append("ms_per_step (first start to last end / K): %.3f" % ((last - first) / 1e6 / steps))
    names = sorted({r["name"] for r in members})
    for n in names:
        k = [r for r in members if r["name"] == n]
        d = [(r["t1"] - r["t0"]) / 1e6 for r in k]
        out.append("  %-70s x%-3d mean %.3f ms (min %.3f, max %.3f) lds %s vgpr %s" % (
            n[:70], len(k), statistics.mean(d), min(d), max(d), k[0]["lds"], k[0]["vgpr"]))
    out.append("step  queue  chain  table: wait_ms  dur_ms  before_other_search_end_ms (share of it)  | search dur_ms")
    waits, befores, shares = [], [], []
    for i, (s, prev_end, chain, table) in enumerate(per_step):
        line = "%4d  %5s  %5d  " % (i, s["q"], len(chain))
        if table is None:
            line += "no table kernel"
        else:
            wait = (table["t0"] - prev_end) / 1e6 if prev_end is not None else float("nan")
            other = [o for o in searches if o["q"] != s["q"] and o["t0"] <= table["t0"] < o["t1"]]
            if other:
                o = other[-1]
                before, share = (o["t1"] - table["t0"]) / 1e6, (o["t1"] - table["t0"]) / (o["t1"] - o["t0"])
                befores.append(before)
                shares.append(share)
                tail = "%8.3f (%.2f)" % (before, share)
            else:
                tail = "no search running on the other queue"
            if i >= 2:
                waits.append(wait)
            line += "%12.3f  %6.3f  %s" % (wait, (table["t1"] - table["t0"]) / 1e6, tail)
        line += "  | %.3f" % ((s["t1"] - s["t0"]) / 1e6)
        out.append(line)
    if waits:
        out.append("table wait after becoming eligible, steps 2..: median %.3f ms, max %.3f ms" % (
            statistics.median(waits), max(waits)))
    if befores:
        out.append("table start before the end of the other lane's search: median %.3f ms (share %.2f)" % (
            statistics.median(befores), statistics.median(shares)))
    ss, ts = [], []
    for i, a in enumerate(timed):
        for b in timed[i + 1:]:
            if overlap(a, b):
                ss.append((max(a["t0"], b["t0"]), min(a["t1"], b["t1"])))
    for _, _, _, table in per_step:
        if table is None:
            continue
        for b in searches:
            if b["q"] != table["q"] and overlap(table, b):
                ts.append((max(table["t0"], b["t0"]), min(table["t1"], b["t1"])))
    out.append("search + search resident together: %.3f ms per step" % (union_ms(ss) / steps))
    out.append("table + search resident together:  %.3f ms per step" % (union_ms(ts) / steps))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", help="rocprofv3 kernel-trace CSV")
    ap.add_argument("--steps", type=int, default=20, help="K of the traced bench.py run")
    args = ap.parse_args()
    print(summarize(read_trace(args.trace), args.steps))


if __name__ == "__main__":
    sys.exit(main())
