"""The exact top-k for a TABLE of allow-lists grouped by bitmap (phnsw_search_exact_grouped_device) beside the two things a
caller could do without it, on the bench.py data: the 1M x 768 clustered "survey" set, 10 000 device-resident queries,
one stream, k = 10.  The exact calls never walk the graph, so the index is an adopted one-layer ring (no build).

One cell per (nfilters, density per bitmap); the queries are spread evenly over the bitmaps and interleaved
(filter_of[q] = q % nfilters).  Per cell three variants are timed ALTERNATELY inside this one run, --runs rounds (five at
least), each round --warmup + --steps launches per variant between two device events; median and spread (max - min) of
the rounds' ms per step are reported:

  grouped  the new call
  scan     the only single call there was: phnsw_search_exact_filtered_device with per-query bitmaps, the table
           replicated per query beforehand (not timed; 1.25 GB at 1M rows and 10 000 queries)
  split    the best a caller could do: the queries gathered by bitmap beforehand (not timed), then one
           phnsw_search_exact_shared_device per bitmap; scattering the rows back is not timed either

`grouped` and every call of `split` synchronise the stream once by contract; that wait is inside their times.  The rows
of `grouped` are compared with the rows of `scan` and, scattered back, of `split` at full size (ids, distance bits,
lengths: they must be equal).  The steps of `grouped` (group, count, list, pack + table, select) come from the library's
own events: one extra call per cell with PHNSW_GROUP_TIMES=1, which prints them to stderr (captured here).  One JSON line
per cell.

  python scripts/bench_filter_grouped.py [--cells 1:0.01,8:0.01,64:0.01,1000:0.01,8:0.001,8:0.1] [--out FILE]"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_filter_dense import captured_stderr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="1:0.01,8:0.01,64:0.01,1000:0.01,8:0.001,8:0.1", help="nfilters:density, ...")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
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
    ring = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + n - 1) % n], axis=1).astype(np.uint64)
    index = ph.Hnsw.from_layers(full, [(np.arange(n, dtype=np.uint64), ring)])
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    ld = qs.ld
    padded = np.zeros((nq, ld), dtype=np.float32)  # the queries as a tensor: `split` gathers them
    padded[:, :dim] = qs.read()[:, :dim]
    qrows = torch.from_numpy(padded).to(dev)
    stream = torch.cuda.Stream()
    nw = (n + 31) // 32

    def outputs(rows):
        return (torch.empty((rows, k), dtype=torch.int32, device=dev), torch.empty((rows, k), dtype=torch.float32, device=dev),
                torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev))

    out = {v: outputs(nq) for v in ("grouped", "scan", "split")}
    lines = []
    for cell in args.cells.split(","):
        nf, density = int(cell.split(":")[0]), float(cell.split(":")[1])
        gen = torch.Generator(device=dev).manual_seed(7)
        table = torch.zeros((nf, nw), dtype=torch.int32, device=dev)  # bits drawn on the device, 32 ids per word
        for b in range(32):
            bit = (torch.rand((nf, nw), generator=gen, device=dev) < density).to(torch.int32)
            table |= bit << b if b < 31 else bit * -(2 ** 31)
        filter_of = (torch.arange(nq, device=dev) % nf).to(torch.int32)
        per_query = table[filter_of.long()].contiguous()  # [nq, nw]: what the scan needs
        order = torch.argsort(filter_of.long(), stable=True)
        gathered = qrows[order].contiguous()
        bounds = np.searchsorted(filter_of.cpu().numpy()[order.cpu().numpy()], np.arange(nf + 1))
        counts = torch.zeros(nf, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        index.filter_count_device(nf, counts.data_ptr(), allow=table.data_ptr(), allow_stride=nw)
        torch.cuda.synchronize()
        cand = counts.cpu().numpy().view(np.uint32).astype(np.int64)
        pairs = int(sum(int(cand[f]) * int(bounds[f + 1] - bounds[f]) for f in range(nf)))

        def grouped():
            ids, d, ln, st = out["grouped"]
            index.search_exact_grouped_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                              queries=qrows.data_ptr(), ldq=ld, allows=table.data_ptr(), allow_stride=nw,
                                              nallows=nf, allow_of=filter_of.data_ptr(), stream=stream.cuda_stream)

        def scan():
            ids, d, ln, st = out["scan"]
            index.search_exact_filtered_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                               queries=qrows.data_ptr(), ldq=ld, allow=per_query.data_ptr(), allow_stride=nw,
                                               stream=stream.cuda_stream)

        def split():
            ids, d, ln, st = out["split"]  # rows in gathered order
            for f in range(nf):
                a, b = int(bounds[f]), int(bounds[f + 1])
                if a == b:
                    continue
                index.search_exact_shared_device(b - a, k, ids[a:].data_ptr(), d[a:].data_ptr(), ln[a:].data_ptr(),
                                                 st[a:].data_ptr(), queries=gathered[a:].data_ptr(), ldq=ld,
                                                 allow=table[f].data_ptr(), stream=stream.cuda_stream)

        def timed(name, launch):
            for _ in range(args.warmup):
                launch()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.steps):
                launch()
            b.record(stream)
            torch.cuda.synchronize()
            assert not out[name][3].cpu().numpy().any(), "a query failed"
            return round(a.elapsed_time(b) / args.steps, 4)

        variants = (("grouped", grouped), ("scan", scan), ("split", split))
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all three
            for v, f in variants:
                runs[v].append(timed(v, f))
        g, s, p = ([x.cpu().numpy() for x in out[v][:3]] for v in ("grouped", "scan", "split"))
        back = np.empty(nq, dtype=np.int64)
        back[order.cpu().numpy()] = np.arange(nq)
        p = [x[back] for x in p]  # the rows of `split`, scattered back

        def rows_equal(x, y):
            return bool((x[0] == y[0]).all() and (x[1].view(np.uint32) == y[1].view(np.uint32)).all() and (x[2] == y[2]).all())

        os.environ["PHNSW_GROUP_TIMES"] = "1"
        try:
            text = captured_stderr(lambda: (grouped(), torch.cuda.synchronize()))
        finally:
            del os.environ["PHNSW_GROUP_TIMES"]
        m = re.search(r"(\d+) groups in (\d+) rounds, (\d+) listed candidates: group ([\d.]+) ms, count ([\d.]+) ms, "
                      r"list ([\d.]+) ms, pack\+table ([\d.]+) ms, select ([\d.]+) ms", text)
        steps = None
        if m:
            steps = dict(zip(("groups", "rounds", "listed"), map(int, m.groups()[:3])))
            steps.update(zip(("group", "count", "list", "pack_table", "select"), map(float, m.groups()[3:])))
        line = {"nfilters": nf, "density": density, "vectors": n, "dim": dim, "queries": nq, "k": k,
                "candidates_per_bitmap": {"min": int(cand.min()), "max": int(cand.max())}, "pairs": pairs, "steps": args.steps,
                "warmup": args.warmup, "rounds": args.runs, "grouped_rows_equal_scan_rows": rows_equal(g, s),
                "grouped_rows_equal_split_rows": rows_equal(g, p), "grouped_steps_ms": steps}
        for v, _ in variants:
            med = float(np.median(runs[v]))
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": med, "spread": round(max(runs[v]) - min(runs[v]), 4)}
        line["scan_over_grouped"] = round(line["scan_ms_per_step"]["median"] / line["grouped_ms_per_step"]["median"], 3)
        line["split_over_grouped"] = round(line["split_ms_per_step"]["median"] / line["grouped_ms_per_step"]["median"], 3)
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        assert line["grouped_rows_equal_scan_rows"] and line["grouped_rows_equal_split_rows"], "rows differ at %s" % cell
        del table, per_query, gathered
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
