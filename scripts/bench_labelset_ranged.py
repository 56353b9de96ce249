"""The three calls by a set of row labels and a numeric range (phnsw_search_exact_labelset_ranged_device,
phnsw_search_batch_labelset_ranged_device, phnsw_search_labelset_ranged_auto_device) beside their bitmap equivalents, on
the bench.py workload: the 1M x 768 clustered set with the same seeds and build, cosine, ef 256 / probe_depth 8, 10 000
device-resident queries, k = 10, one stream.

Every row carries one of --labels labels, drawn at random, and a key that is its rank inside its label in a random order
(distinct keys per label, span order unrelated to id order).  One cell per set size (default 1, 4 and 32 labels): query q
wants that many distinct labels drawn at random and the range [s_q, s_q + c - 1], c = --keep (default a tenth) of the
smallest label's rows and s_q drawn at random: about a tenth of each of its labels.  Per cell the variants are timed
ALTERNATELY inside this one run, --runs rounds, each round --warmup + --steps launches per variant between two device
events; median and spread (max - min) of the rounds' ms per step are reported:

  exact / exact_bitmap   search_exact_labelset_ranged_device / search_exact_filtered_device with the per-query bitmaps of
                         the (set, range) already on the device (ceil(n / 32) words per query)
  walk / walk_bitmap     search_batch_labelset_ranged_device / search_batch_filtered_device, strict
  auto / auto_bitmap     search_labelset_ranged_device / search_filtered_device, each with its library scan_below
  *_up                   the same six with the upload of what describes the filter counted, from pinned host memory on the
                         call's stream in front of every launch: 4 (nq + 1) + 4 nwant + 8 nq bytes against nq bitmaps

The rows of the exact and the walk pairs are compared (ids, distance bits, lengths; stats for the walks): they must be
equal (the two routed calls run with different library thresholds, so their routes may differ).  Bitmap
variants are skipped when nq bitmaps do not fit --bitmap-gb.

--crossover SIZES (candidates of the UNION, e.g. 2000,5000,10000,20000,30000,50000; sets of --crossover-set labels) first
times exact and walk alone with the range cut so that a set holds that many rows: the largest size at which the scan
still wins is filter_route.h's PH_AUTO_SCAN_BELOW_LABELSET_RANGED (--sets "" runs nothing else).  One JSON line per cell.

  python scripts/bench_labelset_ranged.py [--sets 1,4,32] [--keep 0.1] [--crossover SIZES] [--crossover-set 4]
                                          [--labels 64] [--index-file FILE] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1,4,32", help="labels per set, one cell each")
    ap.add_argument("--keep", type=float, default=0.1, help="the part of the smallest label's rows a range keeps of each label")
    ap.add_argument("--crossover", default="", help="candidates of the union: exact and walk alone, one cell each")
    ap.add_argument("--crossover-set", type=int, default=4, help="labels per set in the crossover cells")
    ap.add_argument("--labels", type=int, default=64, help="distinct labels; a set cannot be larger")
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
    cells = [("crossover", args.crossover_set, max(1, int(x) // args.crossover_set)) for x in args.crossover.split(",") if x] + \
        [("cell", int(x), max(1, int(round(args.keep * smallest)))) for x in args.sets.split(",") if x]
    for mode, m, c in cells:  # m labels per set, c rows of each
        if c > smallest or m > T:
            print(json.dumps({"mode": mode, "set": m, "span_rows": c, "skipped": "%d labels, the smallest holds %d rows" % (T, smallest)}),
                  flush=True)
            continue
        # m distinct labels per query: the first m of a random order of the labels
        sets64 = torch.argsort(torch.rand((nq, T), generator=gen, device=dev), dim=1)[:, :m].contiguous()
        start = torch.randint(0, smallest - c + 1, (nq,), generator=gen, device=dev)
        first_h = (torch.arange(nq + 1, dtype=torch.int64) * m).to(torch.int32).pin_memory()
        values_h = sets64.to(torch.int32).cpu().reshape(-1).pin_memory()
        lo_h, hi_h = start.to(torch.int32).cpu().pin_memory(), (start + c - 1).to(torch.int32).cpu().pin_memory()
        first, values, lo, hi = (x.to(dev) for x in (first_h, values_h, lo_h, hi_h))
        nwant = nq * m
        with_bitmaps = mode == "cell" and nq * nw * 4 <= args.bitmap_gb * 2 ** 30
        per_query = per_query_h = None
        if with_bitmaps:
            lab = torch.full((nw * 32,), -1, dtype=torch.int64, device=dev)
            key = torch.full((nw * 32,), -1, dtype=torch.int64, device=dev)
            lab[:n], key[:n] = labels, keys  # -1 behind the last row
            weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
            member = torch.zeros((nq, T + 1), dtype=torch.bool, device=dev)  # column T: the rows behind the last
            member.scatter_(1, sets64, True)
            per_query = torch.empty((nq, nw), dtype=torch.int32, device=dev)
            for q0 in range(0, nq, 16):
                s = start[q0:q0 + 16].view(-1, 1)
                inside = member[q0:q0 + 16][:, lab.clamp(min=-1) % (T + 1)] & (key.view(1, -1) >= s) & (key.view(1, -1) < s + c)
                w = (inside.view(-1, nw, 32).to(torch.int64) * weights).sum(2)
                per_query[q0:q0 + 16] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
            del lab, key, member
            per_query_h = torch.empty((nq, nw), dtype=torch.int32).pin_memory()
            per_query_h.copy_(per_query)

        def ptrs(o):
            return o["ids"].data_ptr(), o["d"].data_ptr(), o["ln"].data_ptr(), o["st"].data_ptr()

        common = dict(queries=qrows.data_ptr(), ldq=ld, stream=stream.cuda_stream)
        desc = dict(want_first=first.data_ptr(), want_values=values.data_ptr(), lo=lo.data_ptr(), hi=hi.data_ptr())

        def upload_sets():
            with torch.cuda.stream(stream):
                for dst, src in ((first, first_h), (values, values_h), (lo, lo_h), (hi, hi_h)):
                    dst.copy_(src, non_blocking=True)

        def upload_bitmaps():
            with torch.cuda.stream(stream):
                per_query.copy_(per_query_h, non_blocking=True)

        def exact():
            index.search_exact_labelset_ranged_device(attr, nq, nwant, k, *ptrs(out["exact"]), **desc, **common)

        def exact_bitmap():
            index.search_exact_filtered_device(nq, k, *ptrs(out["exact_bitmap"]), allow=per_query.data_ptr(), allow_stride=nw, **common)

        def walk():
            o = out["walk"]
            index.search_batch_labelset_ranged_device(attr, nq, nwant, sp, *ptrs(o), strict=True, out_stats=o["stats"].data_ptr(),
                                                      **desc, **common)

        def walk_bitmap():
            o = out["walk_bitmap"]
            index.search_batch_filtered_device(nq, sp, *ptrs(o), allow=per_query.data_ptr(), allow_stride=nw, strict=True,
                                               out_stats=o["stats"].data_ptr(), **common)

        def auto():
            o = out["auto"]
            index.search_labelset_ranged_device(attr, nq, nwant, sp, k, *ptrs(o), out_route=o["route"].data_ptr(), **desc, **common)

        def auto_bitmap():
            o = out["auto_bitmap"]
            index.search_filtered_device(nq, sp, k, *ptrs(o), allow=per_query.data_ptr(), allow_stride=nw,
                                         out_route=o["route"].data_ptr(), **common)

        def with_upload(upload, launch):
            def run():
                upload()
                launch()
            return run

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
            assert not out[name.replace("_up", "")]["st"].cpu().numpy().any(), "a query failed"
            return round(a.elapsed_time(b) / args.steps, 4)

        variants = [("exact", exact), ("walk", walk)]
        if mode == "cell":
            variants.append(("auto", auto))
            variants += [(v + "_up", with_upload(upload_sets, f)) for v, f in list(variants)]
        if with_bitmaps:
            bm = [("exact_bitmap", exact_bitmap), ("walk_bitmap", walk_bitmap), ("auto_bitmap", auto_bitmap)]
            variants += bm + [(v + "_up", with_upload(upload_bitmaps, f)) for v, f in bm]
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for v, f in variants:
                runs[v].append(timed(v, f))
        counts = torch.empty(nq, dtype=torch.int32, device=dev)
        attr.count_set_device(nq, nwant, first.data_ptr(), values.data_ptr(), lo.data_ptr(), hi.data_ptr(), counts.data_ptr())
        torch.cuda.synchronize()
        line = {"mode": mode, "set": m, "span_rows": c, "union_rows": float(counts.to(torch.float64).mean()), "vectors": n, "dim": dim,
                "queries": nq, "k": k, "ef": ef, "labels": T, "probe_depth": args.probe_depth,
                "handle": dict(zip(("n", "listed", "nlabels", "longest"), attr.info())), "steps": args.steps, "warmup": args.warmup,
                "rounds": args.runs, "per_query_bitmap_bytes": nq * nw * 4, "set_bytes": 4 * (nq + 1) + 4 * nwant + 8 * nq,
                "bitmap_variants_run": with_bitmaps}
        for v, _ in variants:
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": float(np.median(runs[v])),
                                        "spread": round(max(runs[v]) - min(runs[v]), 4)}
        med = {v: line[v + "_ms_per_step"]["median"] for v, _ in variants}
        wl = out["walk"]["ln"].cpu().numpy().view(np.uint32)
        line["walk_results_per_query"] = round(float(wl.mean()), 2)
        line["exact_over_walk"] = round(med["exact"] / med["walk"], 4)
        if mode == "cell":
            line["auto_over_better_of_walk_and_exact"] = round(med["auto"] / min(med["walk"], med["exact"]), 4)
            line["auto_routes"] = np.bincount(out["auto"]["route"].cpu().numpy().view(np.uint32), minlength=3).tolist()
            full = np.minimum(k, counts.cpu().numpy().view(np.uint32))
            line["auto_complete"] = int((out["auto"]["ln"].cpu().numpy().view(np.uint32) == full).sum())
        if with_bitmaps:
            def equal(a, b, fields):
                return all(bool((out[a][f].cpu().numpy().view(np.uint32) == out[b][f].cpu().numpy().view(np.uint32)).all())
                           for f in fields)
            line["rows_equal"] = {"exact": equal("exact", "exact_bitmap", ("ids", "d", "ln")),
                                  "walk": equal("walk", "walk_bitmap", ("ids", "d", "ln", "stats"))}
            for v in ("exact", "walk", "auto"):
                line[v + "_over_" + v + "_bitmap"] = round(med[v] / med[v + "_bitmap"], 4)
                line[v + "_up_over_" + v + "_bitmap_up"] = round(med[v + "_up"] / med[v + "_bitmap_up"], 4)
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        assert not with_bitmaps or all(line["rows_equal"].values()), "rows differ at sets of %d labels" % m
        del per_query, per_query_h
    attr.close()


if __name__ == "__main__":
    main()
