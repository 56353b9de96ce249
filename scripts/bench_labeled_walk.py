"""The graph walk by row label (phnsw_search_batch_labeled_device) and the routed call by label
(phnsw_search_labeled_auto_device) beside what a label user had before them, on the bench.py workload: the 1M x 768
clustered set with the same seeds and build, ef 256 / probe_depth 8, 10 000 device-resident queries, k = 10, one stream.

One cell per UNIFORM partition of the rows into L labels (label of v = a random permutation of v % L; default L = 2, 8,
64, 1000); the queries are spread evenly over the labels and interleaved (want[q] = q % L).  Per cell the variants are
timed ALTERNATELY inside this one run, --runs rounds, each round --warmup + --steps launches per variant between two
device events; median and spread (max - min) of the rounds' ms per step are reported:

  (a) walk          search_batch_labeled_device, strict
      walk_bitmap   search_batch_filtered_device, strict, with the per-query bitmaps {v : label of v == want[q]} already on
                    the device (ceil(n / 32) words per query: 1.25 GB at 1M rows and 10 000 queries) -- kernel time alone
      walk_bitmap_upload  the same with the bitmaps copied from pinned host memory to the device inside the timed region,
                    as a caller that builds them per batch pays it
  (b) exact         search_exact_labeled_device at k: with (a) the crossover that would set the labeled scan_below default
                    (filter_route.h, PH_AUTO_SCAN_BELOW_LABELED)
  (c) auto          search_labeled_device (phnsw_search_labeled_auto_device) with the library's scan_below, against the
                    better of walk and exact; the routes it took are counted

The rows of walk and walk_bitmap are compared at full size (ids, distance bits, lengths, stats: they must be equal).
walk returns about ef / L results per query (a post-filter); `results_per_query` says how many, `complete` how many
queries got k of them -- exact and auto always do.  Bitmap variants are skipped when nq bitmaps do not fit --bitmap-gb.
One JSON line per cell.

(d), the unfiltered bench.py value on the parent commit and on this one, is bench.py itself on two checkouts, the runs
alternating:  python bench.py --gpus 1 --steps K --warmup W

  python scripts/bench_labeled_walk.py [--labels 2,8,64,1000] [--index-file FILE] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", default="2,8,64,1000", help="labels of the uniform partitions, one cell each")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=256)
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="rounds, the variants alternating inside each")
    ap.add_argument("--bitmap-gb", type=float, default=4.0, help="most device memory the per-query bitmaps may take")
    ap.add_argument("--index-file", default="", help="load the index from here if the file exists, else build and save it")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k, ef = args.n, args.dim, args.nq, args.k, args.ef
    noise = 0.1 * dim ** 0.5
    store = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    if args.index_file and os.path.exists(args.index_file):
        index = ph.Hnsw.deserialize(args.index_file, store)
    else:
        index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
        if args.index_file:
            index.serialize(args.index_file)
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    ld = qs.ld
    padded = np.zeros((nq, ld), dtype=np.float32)
    padded[:, :dim] = qs.read()[:, :dim]
    qrows = torch.from_numpy(padded).to(dev)
    stream = torch.cuda.Stream()
    sp = ph.SearchParameters(ef, ef, args.probe_depth)
    nw = (n + 31) // 32

    def outputs(width, stats=False):
        return dict(ids=torch.empty((nq, width), dtype=torch.int32, device=dev),
                    d=torch.empty((nq, width), dtype=torch.float32, device=dev),
                    ln=torch.empty(nq, dtype=torch.int32, device=dev), st=torch.empty(nq, dtype=torch.int32, device=dev),
                    stats=torch.empty((nq, 2), dtype=torch.int32, device=dev) if stats else None,
                    route=torch.empty(nq, dtype=torch.int32, device=dev))

    out = {"walk": outputs(ef, True), "walk_bitmap": outputs(ef, True), "exact": outputs(k), "auto": outputs(k)}
    out["walk_bitmap_upload"] = out["walk_bitmap"]
    for L in [int(x) for x in args.labels.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(7)
        lab = torch.empty(n, dtype=torch.int64, device=dev)
        lab[torch.randperm(n, generator=gen, device=dev)] = torch.arange(n, device=dev) % L
        column = lab.to(torch.int32)
        want = (torch.arange(nq, device=dev) % L).to(torch.int32)
        torch.cuda.synchronize()
        labels = ph.Labels.from_device(index, column.data_ptr())
        with_bitmaps = nq * nw * 4 <= args.bitmap_gb * 2 ** 30
        per_query = pinned = None
        if with_bitmaps:
            lab32 = torch.full((nw * 32,), -1, dtype=torch.int64, device=dev)
            lab32[:n] = lab
            lab32 = lab32.view(nw, 32)
            weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
            table = torch.empty((L, nw), dtype=torch.int32, device=dev)
            for f in range(L):
                w = ((lab32 == f).to(torch.int64) * weights).sum(1)
                table[f] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
            per_query = table[want.long()].contiguous()  # [nq, nw]
            pinned = per_query.cpu().pin_memory()
            del table, lab32

        def ptrs(o):
            return o["ids"].data_ptr(), o["d"].data_ptr(), o["ln"].data_ptr(), o["st"].data_ptr()

        def walk():
            o = out["walk"]
            index.search_batch_labeled_device(labels, nq, sp, *ptrs(o), queries=qrows.data_ptr(), ldq=ld, want=want.data_ptr(),
                                              strict=True, out_stats=o["stats"].data_ptr(), stream=stream.cuda_stream)

        def walk_bitmap():
            o = out["walk_bitmap"]
            index.search_batch_filtered_device(nq, sp, *ptrs(o), queries=qrows.data_ptr(), ldq=ld, allow=per_query.data_ptr(),
                                               allow_stride=nw, strict=True, out_stats=o["stats"].data_ptr(),
                                               stream=stream.cuda_stream)

        def walk_bitmap_upload():
            with torch.cuda.stream(stream):
                per_query.copy_(pinned, non_blocking=True)
            walk_bitmap()

        def exact():
            o = out["exact"]
            index.search_exact_labeled_device(labels, nq, k, *ptrs(o), queries=qrows.data_ptr(), ldq=ld, want=want.data_ptr(),
                                              stream=stream.cuda_stream)

        def auto():
            o = out["auto"]
            index.search_labeled_device(labels, nq, sp, k, *ptrs(o), queries=qrows.data_ptr(), ldq=ld, want=want.data_ptr(),
                                        out_route=o["route"].data_ptr(), stream=stream.cuda_stream)

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
            assert not out[name]["st"].cpu().numpy().any(), "a query failed"
            return round(a.elapsed_time(b) / args.steps, 4)

        variants = [("walk", walk)]
        if with_bitmaps:
            variants += [("walk_bitmap", walk_bitmap), ("walk_bitmap_upload", walk_bitmap_upload)]
        variants += [("exact", exact), ("auto", auto)]
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for v, f in variants:
                runs[v].append(timed(v, f))
        info = labels.info()
        line = {"labels": L, "rows_per_label": n // L, "vectors": n, "dim": dim, "queries": nq, "k": k, "ef": ef,
                "probe_depth": args.probe_depth, "handle": dict(zip(("n", "nlabels", "listed", "longest"), info)),
                "steps": args.steps, "warmup": args.warmup, "rounds": args.runs,
                "per_query_bitmap_bytes": nq * nw * 4, "want_bytes": nq * 4, "bitmap_variants_run": with_bitmaps}
        for v, _ in variants:
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": float(np.median(runs[v])),
                                        "spread": round(max(runs[v]) - min(runs[v]), 4)}
        med = {v: line[v + "_ms_per_step"]["median"] for v, _ in variants}
        wl = out["walk"]["ln"].cpu().numpy().view(np.uint32)
        line["walk_results_per_query"] = round(float(wl.mean()), 2)
        line["walk_complete"] = int((wl >= k).sum())
        if with_bitmaps:  # (a)
            same = all(bool((out["walk"][f].cpu().numpy().view(np.uint32) == out["walk_bitmap"][f].cpu().numpy().view(np.uint32)).all())
                       for f in ("ids", "d", "ln", "stats"))
            line["walk_rows_equal_walk_bitmap_rows"] = same
            line["walk_over_walk_bitmap"] = round(med["walk"] / med["walk_bitmap"], 4)
            line["walk_over_walk_bitmap_upload"] = round(med["walk"] / med["walk_bitmap_upload"], 4)
        line["walk_over_exact"] = round(med["walk"] / med["exact"], 4)  # (b)
        line["auto_over_better_of_walk_and_exact"] = round(med["auto"] / min(med["walk"], med["exact"]), 4)  # (c)
        line["auto_routes"] = np.bincount(out["auto"]["route"].cpu().numpy().view(np.uint32), minlength=3).tolist()
        line["auto_complete"] = int((out["auto"]["ln"].cpu().numpy().view(np.uint32) >= min(k, n // L)).sum())
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        assert not with_bitmaps or line["walk_rows_equal_walk_bitmap_rows"], "rows differ at %d labels" % L
        labels.close()
        del per_query, pinned, labels


if __name__ == "__main__":
    main()
