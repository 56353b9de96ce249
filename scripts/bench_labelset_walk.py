"""The graph walk by a SET of row labels (phnsw_search_batch_labelset_device) beside what a set user had before it, on the
bench.py workload: the 1M x 768 clustered set with the same seeds and build, ef 256 / probe_depth 8, 10 000
device-resident queries, k = 10, one stream.

One cell per (labels L, set size S): a UNIFORM partition of the rows into L labels (label of v = a random permutation of
v % L) and, per query, S distinct labels drawn at random.  Per cell the variants are timed ALTERNATELY inside this one run,
--runs rounds, each round --warmup + --steps launches per variant between two device events; median and spread (max - min)
of the rounds' ms per step are reported:

  walk_set            search_batch_labelset_device, strict, the CSR table already on the device
  walk_set_upload     the same with want_first / want_values copied from pinned host memory inside the timed region
                      (4 * (nq + 1) + 4 * nwant bytes)
  walk_bitmap         search_batch_filtered_device, strict, with the per-query UNION bitmaps already on the device
                      (ceil(n / 32) words per query: 1.25 GB at 1M rows and 10 000 queries) -- kernel time alone.  This call
                      exists on the parent commit: it is the yardstick
  walk_bitmap_upload  the same with the bitmaps copied from pinned host memory inside the timed region
  walk_label          S == 1 only: search_batch_labeled_device with want[q] = the one label of the set; the difference to
                      walk_set is reported beside the run-to-run spread of both
  exact_set           search_exact_labelset_device at k: with walk_set the crossover that would set
                      PH_AUTO_SCAN_BELOW_LABELSET (filter_route.h); `union_rows` = S * n / L is what it scans per query

The rows of walk_set and walk_bitmap are compared at full size (ids, distance bits, lengths, stats: they must be equal).
One JSON line per cell.

  python scripts/bench_labelset_walk.py [--cells 1000:1,1000:4,1000:32,500:4,200:4,100:4,50:4] [--index-file FILE] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="1000:1,1000:4,1000:32,500:4,200:4,100:4,50:4", help="labels:set size, one cell each")
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
                    stats=torch.empty((nq, 2), dtype=torch.int32, device=dev) if stats else None)

    out = {"walk_set": outputs(ef, True), "walk_bitmap": outputs(ef, True), "walk_label": outputs(ef, True), "exact_set": outputs(k)}
    out["walk_set_upload"], out["walk_bitmap_upload"] = out["walk_set"], out["walk_bitmap"]
    made = {}  # per L: the column, its handle and the table of per-label bitmaps
    for cell in args.cells.split(","):
        L, S = (int(x) for x in cell.split(":"))
        if L not in made:
            for old in made.values():
                old[1].close()
            made.clear()
            gen = torch.Generator(device=dev).manual_seed(7)
            lab = torch.empty(n, dtype=torch.int64, device=dev)
            lab[torch.randperm(n, generator=gen, device=dev)] = torch.arange(n, device=dev) % L
            column = lab.to(torch.int32)
            torch.cuda.synchronize()
            labels = ph.Labels.from_device(index, column.data_ptr())
            lab32 = torch.full((nw * 32,), -1, dtype=torch.int64, device=dev)
            lab32[:n] = lab
            lab32 = lab32.view(nw, 32)
            weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
            table = torch.empty((L, nw), dtype=torch.int32, device=dev)
            for f in range(L):
                w = ((lab32 == f).to(torch.int64) * weights).sum(1)
                table[f] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
            made[L] = (column, labels, table)
            del lab32, lab
        column, labels, table = made[L]
        gen = torch.Generator(device=dev).manual_seed(1000 * L + S)
        sets = torch.rand((nq, L), generator=gen, device=dev).argsort(dim=1)[:, :S].contiguous()  # [nq, S] distinct labels
        first = (torch.arange(nq + 1, device=dev) * S).to(torch.int32)
        values = sets.reshape(-1).to(torch.int32).contiguous()
        nwant = nq * S
        first_pin, values_pin = first.cpu().pin_memory(), values.cpu().pin_memory()
        want1 = sets[:, 0].to(torch.int32).contiguous()
        with_bitmaps = nq * nw * 4 <= args.bitmap_gb * 2 ** 30
        per_query = pinned = None
        if with_bitmaps:
            per_query = table[sets[:, 0]].contiguous()  # [nq, nw]
            for s in range(1, S):
                per_query |= table[sets[:, s]]
            pinned = per_query.cpu().pin_memory()

        def ptrs(o):
            return o["ids"].data_ptr(), o["d"].data_ptr(), o["ln"].data_ptr(), o["st"].data_ptr()

        def walk_set():
            o = out["walk_set"]
            index.search_batch_labelset_device(labels, nq, nwant, sp, *ptrs(o), queries=qrows.data_ptr(), ldq=ld,
                                               want_first=first.data_ptr(), want_values=values.data_ptr(), strict=True,
                                               out_stats=o["stats"].data_ptr(), stream=stream.cuda_stream)

        def walk_set_upload():
            with torch.cuda.stream(stream):
                first.copy_(first_pin, non_blocking=True)
                values.copy_(values_pin, non_blocking=True)
            walk_set()

        def walk_bitmap():
            o = out["walk_bitmap"]
            index.search_batch_filtered_device(nq, sp, *ptrs(o), queries=qrows.data_ptr(), ldq=ld, allow=per_query.data_ptr(),
                                               allow_stride=nw, strict=True, out_stats=o["stats"].data_ptr(),
                                               stream=stream.cuda_stream)

        def walk_bitmap_upload():
            with torch.cuda.stream(stream):
                per_query.copy_(pinned, non_blocking=True)
            walk_bitmap()

        def walk_label():
            o = out["walk_label"]
            index.search_batch_labeled_device(labels, nq, sp, *ptrs(o), queries=qrows.data_ptr(), ldq=ld, want=want1.data_ptr(),
                                              strict=True, out_stats=o["stats"].data_ptr(), stream=stream.cuda_stream)

        def exact_set():
            o = out["exact_set"]
            index.search_exact_labelset_device(labels, nq, nwant, k, *ptrs(o), queries=qrows.data_ptr(), ldq=ld,
                                               want_first=first.data_ptr(), want_values=values.data_ptr(),
                                               stream=stream.cuda_stream)

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

        variants = [("walk_set", walk_set), ("walk_set_upload", walk_set_upload)]
        if with_bitmaps:
            variants += [("walk_bitmap", walk_bitmap), ("walk_bitmap_upload", walk_bitmap_upload)]
        if S == 1:
            variants += [("walk_label", walk_label)]
        variants += [("exact_set", exact_set)]
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for v, f in variants:
                runs[v].append(timed(v, f))
        line = {"labels": L, "set_size": S, "rows_per_label": n // L, "union_rows": S * (n // L), "vectors": n, "dim": dim,
                "queries": nq, "k": k, "ef": ef, "probe_depth": args.probe_depth, "steps": args.steps, "warmup": args.warmup,
                "rounds": args.runs, "per_query_bitmap_bytes": nq * nw * 4, "set_bytes": 4 * (nq + 1) + 4 * nwant,
                "bitmap_variants_run": with_bitmaps}
        for v, _ in variants:
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": float(np.median(runs[v])),
                                        "spread": round(max(runs[v]) - min(runs[v]), 4)}
        med = {v: line[v + "_ms_per_step"]["median"] for v, _ in variants}
        wl = out["walk_set"]["ln"].cpu().numpy().view(np.uint32)
        line["walk_results_per_query"] = round(float(wl.mean()), 2)
        line["walk_complete"] = int((wl >= k).sum())

        def rows_equal(a, b):
            return all(bool((out[a][f].cpu().numpy().view(np.uint32) == out[b][f].cpu().numpy().view(np.uint32)).all())
                       for f in ("ids", "d", "ln", "stats"))

        if with_bitmaps:
            line["walk_set_rows_equal_walk_bitmap_rows"] = rows_equal("walk_set", "walk_bitmap")
            line["walk_set_over_walk_bitmap"] = round(med["walk_set"] / med["walk_bitmap"], 4)
            line["walk_set_upload_over_walk_bitmap_upload"] = round(med["walk_set_upload"] / med["walk_bitmap_upload"], 4)
        if S == 1:
            line["walk_set_rows_equal_walk_label_rows"] = rows_equal("walk_set", "walk_label")
            line["walk_set_minus_walk_label_ms"] = round(med["walk_set"] - med["walk_label"], 4)
        line["walk_set_over_exact_set"] = round(med["walk_set"] / med["exact_set"], 4)
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        assert not with_bitmaps or line["walk_set_rows_equal_walk_bitmap_rows"], "rows differ at %d labels, sets of %d" % (L, S)
        del per_query, pinned


if __name__ == "__main__":
    main()
