"""The exact scan over an allow-list (phnsw_search_exact_filtered_device) beside the graph's filtered search
(phnsw_search_batch_filtered_device, strict) on the bench.py workload: the 1M x 768 clustered "survey" set, the same
seeds and build, 10 000-query batches, device-resident, one stream.  Cells:

  shared_0.1 / shared_0.01 / shared_0.001     one allow bitmap of that density for the whole batch
  per_query_0.01                              one bitmap per query

Per cell and per method (`exact` at k = 10; `graph` at ef = min(10 / density, 1024), probe_depth 8, strict): ms per step
from device events after warm-up, --runs repetitions taken ALTERNATELY (exact, graph, exact, graph, ...) with the spread
beside the median; queries per second; results returned per query; for the graph search recall@10 against the exact
result.  For the scan also the candidates per query (phnsw_filter_count_device) and its algorithmic bytes
(nq x candidates x row bytes) per second as a fraction of the HBM peak (--hbm-gbs, 8000 by default).  One JSON line per
cell and method.

  python scripts/bench_filter_exact.py [--cells shared_0.1,shared_0.01,shared_0.001,per_query_0.01] [--out FILE]

The L2 hit rate of the scan is not taken here: counters are collected in a run of their own,
  rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum -d OUT -- python scripts/bench_filter_exact.py --cells shared_0.01 --only exact --runs 1 --steps 2 --warmup 1
(no tracing option beside --pmc), summed over the ph_exact_scan_kernel dispatches (profiles/filter_exact/README.md)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="shared_0.1,shared_0.01,shared_0.001,per_query_0.01")
    ap.add_argument("--only", default="", help="exact or graph: time one method only")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of every timed measurement, the methods alternating")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM peak the scan's algorithmic bytes are set against")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, args.k
    noise = 0.1 * dim ** 0.5
    store = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    stream = torch.cuda.Stream()
    nw = (n + 31) // 32
    row_bytes = store.ld * 4
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    x_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    x_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    x_ln = torch.empty(nq, dtype=torch.int32, device=dev)
    out_lines = []
    for cell in args.cells.split(","):
        density = float(cell.rsplit("_", 1)[1])
        rows = nq if cell.startswith("per_query") else 1
        gen = torch.Generator(device=dev).manual_seed(7)
        words = torch.zeros((rows, nw), dtype=torch.int32, device=dev)  # bits drawn on the device, 32 ids per word
        for b in range(32):
            bit = (torch.rand((rows, nw), generator=gen, device=dev) < density).to(torch.int32)
            words |= bit << b if b < 31 else bit * -(2 ** 31)
        stride = nw if rows > 1 else 0
        counts = torch.zeros(rows, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        index.filter_count_device(rows, counts.data_ptr(), allow=words.data_ptr(), allow_stride=stride)
        torch.cuda.synchronize()
        candidates = float(counts.cpu().numpy().view(np.uint32).astype(np.float64).mean())
        ef = int(min(max(round(k / density), k), 1024))
        sp = ph.SearchParameters(ef, ef, args.probe_depth)
        g_ids = torch.empty((nq, ef), dtype=torch.int32, device=dev)
        g_d = torch.empty((nq, ef), dtype=torch.float32, device=dev)
        g_ln = torch.empty(nq, dtype=torch.int32, device=dev)

        def exact():
            index.search_exact_filtered_device(nq, k, x_ids.data_ptr(), x_d.data_ptr(), x_ln.data_ptr(), status.data_ptr(),
                                               queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=stride,
                                               stream=stream.cuda_stream)

        def graph():
            index.search_batch_filtered_device(nq, sp, g_ids.data_ptr(), g_d.data_ptr(), g_ln.data_ptr(), status.data_ptr(),
                                               queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=stride,
                                               strict=True, stream=stream.cuda_stream)

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

        methods = [(m, f) for m, f in (("exact", exact), ("graph", graph)) if not args.only or args.only == m]
        runs = {m: [] for m, _ in methods}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on both methods
            for m, f in methods:
                runs[m].append(timed(f))
        xi = x_ids.cpu().numpy().view(np.uint32)
        for m, _ in methods:
            med = float(np.median(runs[m]))
            line = {"cell": cell, "method": m, "density": density, "vectors": n, "dim": dim, "queries": nq, "k": k,
                    "candidates_per_query": round(candidates, 1), "steps": args.steps, "warmup": args.warmup,
                    "ms_per_step": {"runs": runs[m], "median": med, "spread": round(max(runs[m]) - min(runs[m]), 4)},
                    "queries_per_second": round(nq / med * 1000.0, 1)}
            if m == "exact":
                gbs = nq * candidates * row_bytes / (med * 1e-3) / 1e9
                line.update(results_per_query=round(float(x_ln.cpu().numpy().astype(np.int64).mean()), 2),
                            algorithmic_gb_per_second=round(gbs, 1), fraction_of_hbm_peak=round(gbs / args.hbm_gbs, 4))
            else:
                gl = np.minimum(g_ln.cpu().numpy().astype(np.int64), k)
                gi = g_ids.cpu().numpy().view(np.uint32)[:, :k]
                line.update(ef=ef, probe_depth=args.probe_depth, results_per_query=round(float(gl.mean()), 2))
                if "exact" in runs:  # recall@10 of the graph search against the exact result
                    xl = x_ln.cpu().numpy().astype(np.int64)
                    hit = sum(len(set(gi[i, :gl[i]].tolist()) & set(xi[i, :xl[i]].tolist())) for i in range(nq))
                    line["recall_at_k"] = round(hit / max(int(xl.sum()), 1), 4)
            print(json.dumps(line), flush=True)
            out_lines.append(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
