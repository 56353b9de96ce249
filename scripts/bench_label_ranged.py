"""The three calls by a row label and a numeric range (phnsw_search_exact_label_ranged_device,
phnsw_search_batch_label_ranged_device, phnsw_search_label_ranged_auto_device) beside their bitmap equivalents, on the
bench.py workload: the 1M x 768 clustered set with the same seeds and build, cosine, ef 256 / probe_depth 8, 10 000
device-resident queries, k = 10, one stream.

Every row carries one of --labels labels, drawn at random, and a key that is its rank inside its label in a random
order (distinct keys per label, span order unrelated to id order); query q asks for a random label and [s_q, s_q + c -
1], s_q drawn at random below the smallest label's size: a span of exactly c rows placed at random.  One cell per span
size (default 0.1 %, 1 %, 2 %, 5 % and 20 % of the rows).  Per cell the variants are timed ALTERNATELY inside this one
run, --runs rounds, each round --warmup + --steps launches per variant between two device events; median and spread
(max - min) of the rounds' ms per step are reported:

  exact / exact_bitmap   search_exact_label_ranged_device / search_exact_filtered_device with the per-query bitmaps of
                         the pairs already on the device (ceil(n / 32) words per query)
  walk / walk_bitmap     search_batch_label_ranged_device / search_batch_filtered_device, strict
  auto / auto_bitmap     search_label_ranged_device / search_filtered_device, each with its library scan_below

The rows of every pair are compared (ids, distance bits, lengths; stats for the walks): they must be equal.  Bitmap
variants are skipped when nq bitmaps do not fit --bitmap-gb.

--crossover SIZES (rows, e.g. 2000,5000,10000,20000,30000,50000) first times exact and walk alone at those span sizes:
the largest size at which the scan still wins is filter_route.h's PH_AUTO_SCAN_BELOW_LABEL_RANGED (--fractions "" runs
nothing else).  One JSON line per cell.

  python scripts/bench_label_ranged.py [--fractions 0.001,0.01,0.02,0.05,0.2] [--crossover SIZES] [--labels 4]
                                       [--index-file FILE] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fractions", default="0.001,0.01,0.02,0.05,0.2", help="span sizes as fractions of the rows, one cell each")
    ap.add_argument("--crossover", default="", help="span sizes in rows: exact and walk alone, one cell each")
    ap.add_argument("--labels", type=int, default=4, help="distinct labels; the largest span must fit the smallest label")
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
    n, dim, nq, k, ef, T = args.n, args.dim, args.nq, args.k, args.ef, args.labels
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
    gen = torch.Generator(device=dev).manual_seed(7)
    labels = torch.randint(0, T, (n,), generator=gen, device=dev)  # i64
    order = torch.argsort(labels * n + torch.randperm(n, generator=gen, device=dev))  # by label, random inside one
    sizes = torch.bincount(labels, minlength=T)
    starts = torch.cumsum(sizes, 0) - sizes
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    keys[order] = torch.arange(n, device=dev) - starts[labels[order]]  # the rank inside the label
    smallest = int(sizes.min())
    lab32, key32col = labels.to(torch.int32), keys.to(torch.int32)
    torch.cuda.synchronize()
    attr = ph.LabeledAttribute.from_device(index, lab32.data_ptr(), key32col.data_ptr(), dtype=np.uint32)

    def outputs(width, stats=False):
        return dict(ids=torch.empty((nq, width), dtype=torch.int32, device=dev),
                    d=torch.empty((nq, width), dtype=torch.float32, device=dev),
                    ln=torch.empty(nq, dtype=torch.int32, device=dev), st=torch.empty(nq, dtype=torch.int32, device=dev),
                    stats=torch.empty((nq, 2), dtype=torch.int32, device=dev) if stats else None,
                    route=torch.empty(nq, dtype=torch.int32, device=dev))

    out = {"walk": outputs(ef, True), "walk_bitmap": outputs(ef, True), "exact": outputs(k), "exact_bitmap": outputs(k),
           "auto": outputs(k), "auto_bitmap": outputs(k)}
    cells = [("crossover", int(x)) for x in args.crossover.split(",") if x] + \
        [("cell", max(1, int(round(float(x) * n)))) for x in args.fractions.split(",") if x]
    for mode, c in cells:
        if c > smallest:
            print(json.dumps({"mode": mode, "span_rows": c, "skipped": "the smallest label holds %d rows" % smallest}), flush=True)
            continue
        want64 = torch.randint(0, T, (nq,), generator=gen, device=dev)
        start = torch.randint(0, smallest - c + 1, (nq,), generator=gen, device=dev)
        want, lo, hi = want64.to(torch.int32), start.to(torch.int32), (start + c - 1).to(torch.int32)
        with_bitmaps = mode == "cell" and nq * nw * 4 <= args.bitmap_gb * 2 ** 30
        per_query = None
        if with_bitmaps:
            comp = torch.full((nw * 32,), -1, dtype=torch.int64, device=dev)
            comp[:n] = labels * (2 ** 32) + keys  # the composite; -1 behind the last row
            comp = comp.view(1, nw, 32)
            weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
            per_query = torch.empty((nq, nw), dtype=torch.int32, device=dev)
            for q0 in range(0, nq, 32):
                s = (want64[q0:q0 + 32] * (2 ** 32) + start[q0:q0 + 32]).view(-1, 1, 1)
                w = (((comp >= s) & (comp < s + c)).to(torch.int64) * weights).sum(2)
                per_query[q0:q0 + 32] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
            del comp

        def ptrs(o):
            return o["ids"].data_ptr(), o["d"].data_ptr(), o["ln"].data_ptr(), o["st"].data_ptr()

        common = dict(queries=qrows.data_ptr(), ldq=ld, stream=stream.cuda_stream)
        pair = dict(want=want.data_ptr(), lo=lo.data_ptr(), hi=hi.data_ptr())

        def exact():
            index.search_exact_label_ranged_device(attr, nq, k, *ptrs(out["exact"]), **pair, **common)

        def exact_bitmap():
            index.search_exact_filtered_device(nq, k, *ptrs(out["exact_bitmap"]), allow=per_query.data_ptr(), allow_stride=nw, **common)

        def walk():
            o = out["walk"]
            index.search_batch_label_ranged_device(attr, nq, sp, *ptrs(o), strict=True, out_stats=o["stats"].data_ptr(), **pair,
                                                   **common)

        def walk_bitmap():
            o = out["walk_bitmap"]
            index.search_batch_filtered_device(nq, sp, *ptrs(o), allow=per_query.data_ptr(), allow_stride=nw, strict=True,
                                               out_stats=o["stats"].data_ptr(), **common)

        def auto():
            o = out["auto"]
            index.search_label_ranged_device(attr, nq, sp, k, *ptrs(o), out_route=o["route"].data_ptr(), **pair, **common)

        def auto_bitmap():
            o = out["auto_bitmap"]
            index.search_filtered_device(nq, sp, k, *ptrs(o), allow=per_query.data_ptr(), allow_stride=nw,
                                         out_route=o["route"].data_ptr(), **common)

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

        variants = [("exact", exact), ("walk", walk)]
        if mode == "cell":
            variants.append(("auto", auto))
        if with_bitmaps:
            variants += [("exact_bitmap", exact_bitmap), ("walk_bitmap", walk_bitmap), ("auto_bitmap", auto_bitmap)]
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for v, f in variants:
                runs[v].append(timed(v, f))
        line = {"mode": mode, "span_rows": c, "vectors": n, "dim": dim, "queries": nq, "k": k, "ef": ef, "labels": T,
                "probe_depth": args.probe_depth, "handle": dict(zip(("n", "listed", "nlabels", "longest"), attr.info())),
                "steps": args.steps, "warmup": args.warmup, "rounds": args.runs,
                "per_query_bitmap_bytes": nq * nw * 4, "pair_bytes": nq * 12, "bitmap_variants_run": with_bitmaps}
        for v, _ in variants:
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": float(np.median(runs[v])),
                                        "spread": round(max(runs[v]) - min(runs[v]), 4)}
        med = {v: line[v + "_ms_per_step"]["median"] for v, _ in variants}
        wl = out["walk"]["ln"].cpu().numpy().view(np.uint32)
        line["walk_results_per_query"] = round(float(wl.mean()), 2)
        line["walk_complete"] = int((wl >= min(k, c)).sum())
        line["exact_over_walk"] = round(med["exact"] / med["walk"], 4)
        if mode == "cell":
            line["auto_over_better_of_walk_and_exact"] = round(med["auto"] / min(med["walk"], med["exact"]), 4)
            line["auto_routes"] = np.bincount(out["auto"]["route"].cpu().numpy().view(np.uint32), minlength=3).tolist()
            line["auto_complete"] = int((out["auto"]["ln"].cpu().numpy().view(np.uint32) >= min(k, c)).sum())
        if with_bitmaps:
            def equal(a, b, fields):
                return all(bool((out[a][f].cpu().numpy().view(np.uint32) == out[b][f].cpu().numpy().view(np.uint32)).all())
                           for f in fields)
            line["rows_equal"] = {"exact": equal("exact", "exact_bitmap", ("ids", "d", "ln")),
                                  "walk": equal("walk", "walk_bitmap", ("ids", "d", "ln", "stats"))}
            for v in ("exact", "walk", "auto"):
                line[v + "_over_" + v + "_bitmap"] = round(med[v] / med[v + "_bitmap"], 4)
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        assert not with_bitmaps or all(line["rows_equal"].values()), "rows differ at spans of %d rows" % c
        del per_query
    attr.close()


if __name__ == "__main__":
    main()
