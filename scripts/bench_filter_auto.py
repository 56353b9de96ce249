"""The routed filtered search (phnsw_search_filtered_auto_device) beside the two calls it chooses between -- the exact
scan (phnsw_search_exact_filtered_device) and the graph's strict filtered search (phnsw_search_batch_filtered_device) --
on the cells of profiles/filter_exact/README.md: the bench.py workload (1M x 768 clustered rows, the same seeds and
build), 10 000-query batches, k = 10, device-resident, one stream.  Cells:

  shared_<density>       one allow bitmap of that density for the whole batch
  per_query_<density>    one bitmap per query
  mixed_<lo>_<hi>        per-query bitmaps, the first half of the batch at density lo, the second at hi: the case the
                         routed call exists for

Per cell: `exact` at k; `graph` at ef = min(k / density, 1024) (mixed: at the ef of its dense half AND at 1024, the only
width at which its sparse half returns anything), probe_depth 8, strict; `auto` with the graph's search parameters (mixed:
the dense half's) and the library's scan_below.  ms per step from device events after warm-up, --runs repetitions with
the methods ALTERNATING, median and spread; results per query; for auto the routes taken.  One JSON line per cell and
method.

  python scripts/bench_filter_auto.py [--cells ...] [--only exact|graph|auto] [--index-file FILE] [--out FILE]

--index-file keeps the built index between processes (serialize / deserialize), so that a profiled run holds no build
kernels.  The share of the routed call spent outside the two underlying kernels is taken from a run of its own,
  rocprofv3 --kernel-trace --stats -d OUT -o auto --output-format csv -- python scripts/bench_filter_auto.py \\
      --cells mixed_0.001_0.1 --only auto --runs 1 --steps 5 --warmup 1 --skip-count --index-file FILE
and summed with
  python scripts/bench_filter_auto.py --summarise-stats OUT/.../auto_kernel_stats.csv
(count, route and finish kernels against the search, table and scan kernels; what the two synchronisations cost is the
difference between the event time of a step and the kernels' sum)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTING = ("ph_filter_count_kernel", "ph_auto_route_kernel", "ph_auto_finish_kernel")
UNDERLYING = ("ph_search_kernel", "ph_exact_scan_kernel", "ph_exact_merge_kernel", "ph_tiny", "tiny_")


def summarise_stats(path):
    """kernel_stats.csv of a rocprofv3 --kernel-trace --stats run -> the routing kernels' share of the call's kernels"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    name_col = next(c for c in rows[0] if c.lower() in ("name", "kernel_name", "kernelname"))
    total_col = next(c for c in rows[0] if "total" in c.lower())
    calls_col = next(c for c in rows[0] if "calls" in c.lower() or "count" in c.lower())
    routing, underlying, other, detail = 0.0, 0.0, 0.0, {}
    for r in rows:
        name, ns = r[name_col], float(r[total_col])
        if any(k in name for k in ROUTING):
            routing += ns
            detail[name.split("(")[0][:60]] = {"calls": int(float(r[calls_col])), "total_ms": round(ns / 1e6, 4)}
        elif any(k in name for k in UNDERLYING):
            underlying += ns
            detail[name.split("(")[0][:60]] = {"calls": int(float(r[calls_col])), "total_ms": round(ns / 1e6, 4)}
        else:
            other += ns
    print(json.dumps({"routing_ms": round(routing / 1e6, 4), "underlying_ms": round(underlying / 1e6, 4),
                      "other_kernels_ms": round(other / 1e6, 4),
                      "routing_share_of_kernel_time": round(routing / max(routing + underlying, 1.0), 5), "kernels": detail}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="shared_0.001,shared_0.01,shared_0.02,shared_0.03,shared_0.05,shared_0.1,per_query_0.01,"
                                       "mixed_0.001_0.1")
    ap.add_argument("--only", default="", help="exact, graph or auto: time one method only")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--scan-below", type=int, default=0, help="0 = the library's threshold")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of every timed measurement, the methods alternating")
    ap.add_argument("--index-file", default="", help="load the index from here if the file exists, else build and save it")
    ap.add_argument("--skip-count", action="store_true", help="do not count the candidates (a profiled run: no kernel but the call's)")
    ap.add_argument("--summarise-stats", default="", help="a rocprofv3 kernel_stats.csv: print the routing share and exit")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.summarise_stats:
        return summarise_stats(args.summarise_stats)
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, args.k
    noise = 0.1 * dim ** 0.5
    store = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    if args.index_file and os.path.exists(args.index_file):
        index = ph.Hnsw.deserialize(args.index_file, store)
    else:
        index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
        if args.index_file:
            index.serialize(args.index_file)
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    stream = torch.cuda.Stream()
    nw = (n + 31) // 32
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    out_lines = []

    def bitmap(rows, density, seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        words = torch.zeros((rows, nw), dtype=torch.int32, device=dev)  # bits drawn on the device, 32 ids per word
        for b in range(32):
            bit = (torch.rand((rows, nw), generator=gen, device=dev) < density).to(torch.int32)
            words |= bit << b if b < 31 else bit * -(2 ** 31)
        return words

    for cell in args.cells.split(","):
        parts = cell.split("_")
        if cell.startswith("mixed"):
            lo, hi = float(parts[1]), float(parts[2])
            words = torch.cat([bitmap(nq // 2, lo, 7), bitmap(nq - nq // 2, hi, 8)])
            rows, densities = nq, (lo, hi)
        else:
            rows = nq if cell.startswith("per_query") else 1
            words = bitmap(rows, float(parts[-1]), 7)
            densities = (float(parts[-1]),)
        stride = nw if rows > 1 else 0
        candidates = None
        if not args.skip_count:
            counts = torch.zeros(rows, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            index.filter_count_device(rows, counts.data_ptr(), allow=words.data_ptr(), allow_stride=stride)
            torch.cuda.synchronize()
            candidates = round(float(counts.cpu().numpy().view(np.uint32).astype(np.float64).mean()), 1)
        efs = sorted({int(min(max(round(k / d), k), 1024)) for d in densities})  # ascending: the dense half's first
        bufs = {}

        def rows_of(tag, width):
            if (tag, width) not in bufs:
                bufs[(tag, width)] = (torch.empty((nq, width), dtype=torch.int32, device=dev),
                               torch.empty((nq, width), dtype=torch.float32, device=dev),
                               torch.empty(nq, dtype=torch.int32, device=dev))
            return bufs[(tag, width)]

        route = torch.zeros(nq, dtype=torch.int32, device=dev)

        def exact():
            ids, d, ln = rows_of("exact", k)
            index.search_exact_filtered_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                               queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=stride,
                                               stream=stream.cuda_stream)

        def graph_at(ef):
            sp = ph.SearchParameters(ef, ef, args.probe_depth)

            def graph():
                ids, d, ln = rows_of("graph", ef)
                index.search_batch_filtered_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                                   queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=stride,
                                                   strict=True, stream=stream.cuda_stream)
            return graph

        sp_auto = ph.SearchParameters(efs[0], efs[0], args.probe_depth)
        a_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
        a_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
        a_ln = torch.empty(nq, dtype=torch.int32, device=dev)

        def auto():
            index.search_filtered_device(nq, sp_auto, k, a_ids.data_ptr(), a_d.data_ptr(), a_ln.data_ptr(), status.data_ptr(),
                                         queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=stride,
                                         scan_below=args.scan_below, out_route=route.data_ptr(), stream=stream.cuda_stream)

        def timed(launch):
            for _ in range(args.warmup):
                launch()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.steps):
                launch()
            b.record(stream)
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any(), "a query failed"
            return round(a.elapsed_time(b) / args.steps, 4)

        methods = [("exact", exact, None)] + [("graph", graph_at(ef), ef) for ef in efs] + [("auto", auto, efs[0])]
        methods = [m for m in methods if not args.only or args.only == m[0]]
        runs = {(m, ef): [] for m, _, ef in methods}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on every method
            for m, f, ef in methods:
                runs[(m, ef)].append(timed(f))
        for m, _, ef in methods:
            r = runs[(m, ef)]
            med = float(np.median(r))
            line = {"cell": cell, "method": m, "vectors": n, "dim": dim, "queries": nq, "k": k, "candidates_per_query": candidates,
                    "steps": args.steps, "warmup": args.warmup,
                    "ms_per_step": {"runs": r, "median": med, "spread": round(max(r) - min(r), 4)},
                    "queries_per_second": round(nq / med * 1000.0, 1)}
            if m == "exact":
                line["results_per_query"] = round(float(rows_of("exact", k)[2].cpu().numpy().astype(np.int64).mean()), 2)
            elif m == "graph":
                gl = np.minimum(rows_of("graph", ef)[2].cpu().numpy().astype(np.int64), k)
                line.update(ef=ef, probe_depth=args.probe_depth, results_per_query=round(float(gl.mean()), 2))
            else:
                line.update(ef=ef, probe_depth=args.probe_depth, scan_below=args.scan_below,
                            results_per_query=round(float(a_ln.cpu().numpy().astype(np.int64).mean()), 2),
                            routes=np.bincount(route.cpu().numpy().astype(np.int64), minlength=3).tolist())
            print(json.dumps(line), flush=True)
            out_lines.append(json.dumps(line))
        del words, bufs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
