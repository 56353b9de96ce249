"""profiles/r02/search_kernel_summary.json from
  <dir>/trace/**kernel_trace.csv + kernel_stats.csv   rocprofv3 --kernel-trace --stats -- python3 bench.py --role worker ...
  <dir>/bench_trace.json                              the JSON line that worker printed
  <dir>/bench_full.json                               the JSON line of the `python bench.py --full` run (with PMC)
The worker's last `isolated` launches (one per HIP-event reading) are the unit; a launch of the headline batch is
ph_tiny_prep_kernel + 2 x ph_tiny_pack_kernel + ph_tiny_table_mfma_kernel + ph_search_kernel (or prep + ph_tiny_table_kernel +
search when the store is not one the matrix-core table takes)."""
import csv, glob, json, os, sys

d, out_dir = sys.argv[1], sys.argv[2]
isolated = 10


def find(sub, pat):
    r = sorted(glob.glob(os.path.join(d, sub, "**", pat), recursive=True))
    if not r:
        raise SystemExit("missing %s under %s/%s" % (pat, d, sub))
    return r[-1]


trace = json.loads([l for l in open(os.path.join(d, "bench_trace.json")).read().splitlines() if l.startswith("{")][-1])
full = json.loads([l for l in open(os.path.join(d, "bench_full.json")).read().splitlines() if l.startswith("{")][-1])
rows = list(csv.DictReader(open(find("trace", "*kernel_trace.csv"))))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ours = [r for r in rows if any(k in r["Kernel_Name"] for k in ("ph_search_kernel", "ph_tiny_"))]
# walk back from the end: the batch sweep (5 sizes x 5 launches) and the 100k batch follow the isolated launches in
# the worker; identify launches by the prep kernel and keep those whose search dispatch carries the headline grid
launches, cur = [], []
for r in ours:
    if "ph_tiny_prep" in r["Kernel_Name"] and cur:
        launches.append(cur)
        cur = []
    cur.append(r)
if cur:
    launches.append(cur)
nq = trace["queries_per_step_per_gpu"]
head = [L for L in launches if len(L) in (3, 5) and "ph_search_kernel" in L[-1]["Kernel_Name"]]
# the timed steps + isolated launches of the headline share one shape; take the `isolated` ones that follow the timed region
steps = trace["steps"] + trace["warmup"]
sel = head[-(isolated + 200):]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
by_grid = {}
for L in head:
    by_grid.setdefault(L[-1].get("Grid_Size", L[-1].get("Grid_Size_X", "")), []).append(L)
main = max(by_grid.values(), key=len)  # the headline shape is the most frequent one (sweep cells use 8192 queries)
main = [L for L in main if abs(dur(L[-1]) - sorted(dur(x[-1]) for x in main)[len(main) // 2]) / dur(L[-1]) < 0.25]
last = main[-isolated:]


def short(r):
    n = r["Kernel_Name"]
    for k in ("ph_tiny_prep_kernel", "ph_tiny_pack_kernel", "ph_tiny_table_mfma_kernel", "ph_tiny_table_kernel", "ph_search_kernel"):
        if k in n:
            return k
    return n


summary = {
    "command": "rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --role worker " + trace.get("argv", ""),
    "launch": " + ".join(short(r) for r in last[-1]) + " (one isolated launch of the %d-query headline batch)" % nq,
    "launches_averaged": len(last),
    "avg_ms_per_dispatch": {k: sum(dur(r) for L in last for r in L if short(r) == k) / len(last) for k in dict.fromkeys(short(r) for r in last[-1])},
    "avg_ms_sum_of_dispatches": sum(sum(dur(r) for r in L) for L in last) / len(last),
    "avg_ms_first_start_to_last_end": sum((int(L[-1]["End_Timestamp"]) - int(L[0]["Start_Timestamp"])) / 1e6 for L in last) / len(last),
    "search_kernel_name": last[-1][-1]["Kernel_Name"],
    "bench_reported_kernel_ms_same_process": trace["roofline"]["kernel_ms"],
    "bench_reported_dispatches_same_process": trace["roofline"]["dispatches"],
    "bench_value_same_process": trace["value"],
    "plain_run": {"value": full["value"], "ms_per_step": full["ms_per_step"], "kernel_ms": full["roofline"]["kernel_ms"],
                  "roofline": {k: full["roofline"].get(k) for k in ("achieved", "frac", "traffic", "traffic_read", "traffic_write",
                               "traffic_dram_read", "dram_read_gbs", "algorithmic_bytes_per_launch", "algorithmic_gbs", "reuse_factor",
                               "pmc_dispatches", "calibration", "traffic_source", "source_hash")},
                  "config": full["config"]},
    "pmc": {"source_hash": full["roofline"].get("source_hash"), "reuse_factor": full["roofline"].get("reuse_factor"),
            "workload": {"dataset_text": full["config"]["dataset"], "nq": full["queries_per_step_per_gpu"],
                         "ef": full["config"]["number_of_candidates"], "probe_depth": full["config"]["probe_depth"]}},
}
os.makedirs(out_dir, exist_ok=True)
json.dump(summary, open(os.path.join(out_dir, "search_kernel_summary.json"), "w"), indent=1)
open(os.path.join(out_dir, "kernel_stats_bench.csv"), "w").write(open(find("trace", "*kernel_stats.csv")).read())
json.dump(full, open(os.path.join(out_dir, "bench_r02_full.json"), "w"), indent=1)
print(json.dumps({k: summary[k] for k in ("avg_ms_per_dispatch", "avg_ms_sum_of_dispatches", "bench_reported_kernel_ms_same_process")}, indent=1))
