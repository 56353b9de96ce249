"""The exact top-k for a SHARED allow-list as a distance table (phnsw_search_exact_shared_device) beside the exact scan
(phnsw_search_exact_filtered_device, one shared bitmap) and the graph's strict filtered search
(phnsw_search_batch_filtered_device) on the bench.py workload: the 1M x 768 clustered "survey" set, the same seeds and
build, 10 000-query batches, device-resident, one stream, k = 10.  One cell per density of the shared bitmap.

Per cell the three variants -- `table` (the new call), `scan`, `graph` (ef = min(10 / density, 1024), probe_depth 8,
strict: the ef of profiles/filter_exact/) -- are timed ALTERNATELY inside this one run, --runs rounds (five at least),
each round --warmup + --steps launches per variant between two device events; median and spread (max - min) of the
rounds' ms per step are reported, with the candidate count, the rows of `table` compared with the rows of `scan` (ids,
distance bits, lengths: they must be equal), and recall@k of `graph` against them.  `table` synchronises its stream once
per call by contract; that wait is inside its time.

The steps of `table` (count, list, pack + table, select) come from the library's own events: one extra call per cell
with PHNSW_DENSE_TIMES=1, which prints them to stderr (captured here).  Pack and table are one figure: both are enqueued
inside tiny_table.  One JSON line per cell.

  python scripts/bench_filter_dense.py [--densities 0.001,0.01,0.02,0.1,0.3] [--kind f32|f16|i8|i8q] [--out FILE]"""
import argparse
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def captured_stderr(fn):
    """what fn() writes to file descriptor 2 (the library prints from C)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--densities", default="0.001,0.01,0.02,0.1,0.3")
    ap.add_argument("--kind", default="f32", help="store kind searched: f32, f16, i8 or i8q")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5, help="rounds, the three variants alternating inside each")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.runs >= 1
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, args.k
    noise = 0.1 * dim ** 0.5
    full = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    index = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters())
    if args.kind != "f32":
        store = {"f16": ph.F16Store, "i8": ph.I8Store, "i8q": ph.I8QStore}[args.kind].from_full(full)
        index = ph.Hnsw.from_layers(store, [(l.nodes, l.neighbors) for l in index.layers], index.build_parameters)
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    stream = torch.cuda.Stream()
    nw = (n + 31) // 32
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    out = {v: (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
               torch.empty(nq, dtype=torch.int32, device=dev)) for v in ("table", "scan")}
    lines = []
    for density in (float(x) for x in args.densities.split(",")):
        gen = torch.Generator(device=dev).manual_seed(7)
        words = torch.zeros(nw, dtype=torch.int32, device=dev)  # bits drawn on the device, 32 ids per word
        for b in range(32):
            bit = (torch.rand(nw, generator=gen, device=dev) < density).to(torch.int32)
            words |= bit << b if b < 31 else bit * -(2 ** 31)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        index.filter_count_device(1, count.data_ptr(), allow=words.data_ptr())
        torch.cuda.synchronize()
        candidates = int(count.cpu().numpy().view(np.uint32)[0])
        ef = int(min(max(round(k / density), k), 1024))
        sp = ph.SearchParameters(ef, ef, args.probe_depth)
        g_ids = torch.empty((nq, ef), dtype=torch.int32, device=dev)
        g_d = torch.empty((nq, ef), dtype=torch.float32, device=dev)
        g_ln = torch.empty(nq, dtype=torch.int32, device=dev)

        def table():
            ids, d, ln = out["table"]
            index.search_exact_shared_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                             queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), stream=stream.cuda_stream)

        def scan():
            ids, d, ln = out["scan"]
            index.search_exact_filtered_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                               queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=0,
                                               stream=stream.cuda_stream)

        def graph():
            index.search_batch_filtered_device(nq, sp, g_ids.data_ptr(), g_d.data_ptr(), g_ln.data_ptr(), status.data_ptr(),
                                               queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=0,
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

        variants = (("table", table), ("scan", scan), ("graph", graph))
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all three
            for v, f in variants:
                runs[v].append(timed(f))
        t, s = ([x.cpu().numpy() for x in out[v]] for v in ("table", "scan"))
        equal = bool((t[0] == s[0]).all() and (t[1].view(np.uint32) == s[1].view(np.uint32)).all() and (t[2] == s[2]).all())
        xl = s[2].astype(np.int64)
        xi = s[0].view(np.uint32)
        gl = np.minimum(g_ln.cpu().numpy().astype(np.int64), k)
        gi = g_ids.cpu().numpy().view(np.uint32)[:, :k]
        hit = sum(len(set(gi[i, :gl[i]].tolist()) & set(xi[i, :xl[i]].tolist())) for i in range(nq))
        os.environ["PHNSW_DENSE_TIMES"] = "1"
        try:
            text = captured_stderr(lambda: (table(), torch.cuda.synchronize()))
        finally:
            del os.environ["PHNSW_DENSE_TIMES"]
        m = re.search(r"count ([\d.]+) ms, list ([\d.]+) ms, pack\+table ([\d.]+) ms, select ([\d.]+) ms", text)
        steps = dict(zip(("count", "list", "pack_table", "select"), map(float, m.groups()))) if m else None
        line = {"density": density, "kind": args.kind, "vectors": n, "dim": dim, "queries": nq, "k": k, "candidates": candidates,
                "pairs": nq * candidates, "steps": args.steps, "warmup": args.warmup, "rounds": args.runs,
                "table_rows_equal_scan_rows": equal, "table_steps_ms": steps,
                "graph": {"ef": ef, "probe_depth": args.probe_depth, "results_per_query": round(float(gl.mean()), 2),
                          "recall_at_k": round(hit / max(int(xl.sum()), 1), 4)}}
        for v, _ in variants:
            med = float(np.median(runs[v]))
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": med, "spread": round(max(runs[v]) - min(runs[v]), 4)}
        line["table_ns_per_pair"] = round(line["table_ms_per_step"]["median"] * 1e6 / max(nq * candidates, 1), 4)
        line["scan_ns_per_pair"] = round(line["scan_ms_per_step"]["median"] * 1e6 / max(nq * candidates, 1), 4)
        line["scan_over_table"] = round(line["scan_ms_per_step"]["median"] / line["table_ms_per_step"]["median"], 3)
        line["graph_over_table"] = round(line["graph_ms_per_step"]["median"] / line["table_ms_per_step"]["median"], 3)
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        assert equal, "the table path and the scan disagree at density %g" % density
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
