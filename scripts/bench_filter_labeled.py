"""The exact top-k by row label (phnsw_search_exact_labeled_device) beside the two bitmap calls a caller had, on the
bench.py data: the 1M x 768 clustered "survey" set, 10 000 device-resident queries, one stream, k = 10.  The exact calls
never walk the graph, so the index is an adopted one-layer ring (no build).  The method is scripts/bench_filter_grouped.py's.

One cell per (labels, rows per label): a random set of labels * rows vectors carries the labels in turn, the rest carry
none; the queries are spread evenly over the labels and interleaved (want[q] = q % labels).  Per cell the variants are
timed ALTERNATELY inside this one run, --runs rounds (five at least), each round --warmup + --steps launches per variant
between two device events; median and spread (max - min) of the rounds' ms per step are reported:

  labeled    the new call, default knobs (the tile kernel on this f32 store)
  labeled_t1 the new call with PHNSW_LABEL_TILE=1: the per-query list scan only
  scan       phnsw_search_exact_filtered_device with per-query bitmaps, the table of the labels' bitmaps replicated per
             query beforehand (not timed; 1.25 GB at 1M rows and 10 000 queries)
  grouped    phnsw_search_exact_grouped_device over the table of the labels' bitmaps (synchronises once by contract;
             that wait is inside its time)

`scan` and `grouped` are unchanged by the label work: they are the yardsticks.  Making the handle (once per label
column) is timed apart and not part of any step.  The rows of all variants are compared at full size (ids, distance
bits, lengths: they must be equal).  Cells with more than --bitmap-labels labels run the new call alone: the bitmap table
of 100 000 labels over 1M rows would be 12.5 GB.  A vector carries ONE label, so labels * rows cannot exceed the store: 1000
labels over 1M rows are 1000 rows each.  The shape of the cell scripts/bench_filter_grouped.py measured at 166 ms / 42 ms
-- 10 queries per list of about 10 000 rows -- fits 1M rows at a tenth of the batch: 100 labels of 10 000 rows and 1000
queries, the second command below.  One JSON line per cell.

  python scripts/bench_filter_labeled.py [--cells 1:10000,8:10000,64:10000,1000:1000,8:1000,8:100000,100000:10] [--out FILE]
  python scripts/bench_filter_labeled.py --queries 1000 --cells 100:10000 [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="1:10000,8:10000,64:10000,1000:1000,8:1000,8:100000,100000:10", help="labels:rows each, ...")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5, help="rounds, the variants alternating inside each")
    ap.add_argument("--bitmap-labels", type=int, default=1000, help="most labels the bitmap variants are run with")
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
    padded = np.zeros((nq, ld), dtype=np.float32)
    padded[:, :dim] = qs.read()[:, :dim]
    qrows = torch.from_numpy(padded).to(dev)
    stream = torch.cuda.Stream()
    nw = (n + 31) // 32
    NONE = 0xFFFFFFFF

    def outputs(rows):
        return (torch.empty((rows, k), dtype=torch.int32, device=dev), torch.empty((rows, k), dtype=torch.float32, device=dev),
                torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev))

    names = ("labeled", "labeled_t1", "scan", "grouped")
    out = {v: outputs(nq) for v in names}
    for cell in args.cells.split(","):
        nl, each = int(cell.split(":")[0]), int(cell.split(":")[1])
        assert nl * each <= n, cell
        gen = torch.Generator(device=dev).manual_seed(7)
        perm = torch.randperm(n, generator=gen, device=dev)[:nl * each]
        lab = torch.full((n,), -1, dtype=torch.int64, device=dev)
        lab[perm] = torch.arange(nl * each, device=dev) % nl
        column = torch.where(lab < 0, torch.full_like(lab, NONE), lab).to(torch.int32)  # u32 bits
        want = (torch.arange(nq, device=dev) % nl).to(torch.int32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels = ph.Labels.from_device(index, column.data_ptr())
        create_ms = round((time.perf_counter() - t0) * 1e3, 3)
        info = labels.info()
        with_bitmaps = nl <= args.bitmap_labels
        table = per_query = None
        if with_bitmaps:
            lab32 = torch.full((nw * 32,), -1, dtype=torch.int64, device=dev)
            lab32[:n] = lab
            lab32 = lab32.view(nw, 32)
            weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
            table = torch.empty((nl, nw), dtype=torch.int32, device=dev)
            for f in range(nl):
                w = ((lab32 == f).to(torch.int64) * weights).sum(1)
                table[f] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
            per_query = table[want.long()].contiguous()  # [nq, nw]: what the scan needs

        def labeled():
            ids, d, ln, st = out["labeled"]
            index.search_exact_labeled_device(labels, nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                              queries=qrows.data_ptr(), ldq=ld, want=want.data_ptr(), stream=stream.cuda_stream)

        def labeled_t1():
            ids, d, ln, st = out["labeled_t1"]
            os.environ["PHNSW_LABEL_TILE"] = "1"  # read per call, while the call enqueues
            try:
                index.search_exact_labeled_device(labels, nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                                  queries=qrows.data_ptr(), ldq=ld, want=want.data_ptr(), stream=stream.cuda_stream)
            finally:
                del os.environ["PHNSW_LABEL_TILE"]

        def scan():
            ids, d, ln, st = out["scan"]
            index.search_exact_filtered_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                               queries=qrows.data_ptr(), ldq=ld, allow=per_query.data_ptr(), allow_stride=nw,
                                               stream=stream.cuda_stream)

        def grouped():
            ids, d, ln, st = out["grouped"]
            index.search_exact_grouped_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                              queries=qrows.data_ptr(), ldq=ld, allows=table.data_ptr(), allow_stride=nw,
                                              nallows=nl, allow_of=want.data_ptr(), stream=stream.cuda_stream)

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

        variants = [("labeled", labeled), ("labeled_t1", labeled_t1)]
        if with_bitmaps:
            variants += [("scan", scan), ("grouped", grouped)]
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for v, f in variants:
                runs[v].append(timed(v, f))
        rows = {v: [x.cpu().numpy() for x in out[v][:3]] for v, _ in variants}

        def rows_equal(x, y):
            return bool((x[0] == y[0]).all() and (x[1].view(np.uint32) == y[1].view(np.uint32)).all() and (x[2] == y[2]).all())

        line = {"labels": nl, "rows_per_label": each, "vectors": n, "dim": dim, "queries": nq, "k": k,
                "handle": dict(zip(("n", "nlabels", "listed", "longest"), info)), "handle_create_ms": create_ms,
                "pairs": int(nq) * each, "steps": args.steps, "warmup": args.warmup, "rounds": args.runs,
                "bitmap_table_bytes": nl * nw * 4, "bitmap_variants_run": with_bitmaps}
        for v, _ in variants:
            med = float(np.median(runs[v]))
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": med, "spread": round(max(runs[v]) - min(runs[v]), 4)}
            if v != "labeled":
                line["labeled_rows_equal_%s_rows" % v] = rows_equal(rows["labeled"], rows[v])
                line["%s_over_labeled" % v] = round(med / line["labeled_ms_per_step"]["median"], 3)
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        assert all(line["labeled_rows_equal_%s_rows" % v] for v, _ in variants[1:]), "rows differ at %s" % cell
        labels.close()
        del table, per_query, labels


if __name__ == "__main__":
    main()
