"""The exact top-k by a SET of row labels (phnsw_search_exact_labelset_device) beside what a caller had, on the bench.py
data: the 1M x 768 clustered "survey" set, 10 000 device-resident queries, one stream, k = 10, cosine.  The exact calls
never walk the graph, so the index is an adopted one-layer ring (no build).  The method is scripts/bench_filter_labeled.py's.

One cell per (set size, labels, rows per label): a random set of labels * rows vectors carries the labels in turn, the
rest carry none; every query wants `set size` distinct labels drawn at random.  Per cell the variants are timed
ALTERNATELY inside this one run, --runs rounds, each round --warmup + --steps launches per variant between two device
events; median and spread (max - min) of the rounds' ms per step are reported:

  labelset   the new call, default knobs (the tile kernel on this f32 store)
  scan       (a) phnsw_search_exact_filtered_device with the UNION of every query's lists as per-query bitmaps, made
             beforehand (not timed; 1.25 GB at 1M rows and 10 000 queries): what a caller must do today
  labeled    (b) at set size 1 only: phnsw_search_exact_labeled_device -- the price of the pair machinery and of the
             merge that always runs

`scan` and `labeled` are unchanged by this work: they are the yardsticks.  The rows of all variants are compared at
full size (ids, distance bits, lengths: they must be equal).  One JSON line per cell.

  python scripts/bench_labelset.py [--cells 1:1000:1000,2:1000:1000,4:1000:1000,8:1000:1000,32:1000:1000,4:64:10000] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="1:1000:1000,2:1000:1000,4:1000:1000,8:1000:1000,32:1000:1000,4:64:10000",
                    help="set size:labels:rows each, ...")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="rounds, the variants alternating inside each")
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

    out = {v: outputs(nq) for v in ("labelset", "scan", "labeled")}
    made = {}  # (labels, rows each) -> (handle, bitmap table): cells that share a column share them
    for cell in args.cells.split(","):
        size, nl, each = (int(x) for x in cell.split(":"))
        assert nl * each <= n and size <= nl, cell
        if (nl, each) not in made:
            for h, _ in made.values():
                h.close()
            made.clear()
            gen = torch.Generator(device=dev).manual_seed(7)
            perm = torch.randperm(n, generator=gen, device=dev)[:nl * each]
            lab = torch.full((n,), -1, dtype=torch.int64, device=dev)
            lab[perm] = torch.arange(nl * each, device=dev) % nl
            column = torch.where(lab < 0, torch.full_like(lab, NONE), lab).to(torch.int32)  # u32 bits
            torch.cuda.synchronize()
            handle = ph.Labels.from_device(index, column.data_ptr())
            lab32 = torch.full((nw * 32,), -1, dtype=torch.int64, device=dev)
            lab32[:n] = lab
            lab32 = lab32.view(nw, 32)
            weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
            table = torch.empty((nl, nw), dtype=torch.int32, device=dev)
            for f in range(nl):
                w = ((lab32 == f).to(torch.int64) * weights).sum(1)
                table[f] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
            made[(nl, each)] = (handle, table)
        labels, table = made[(nl, each)]
        gen = torch.Generator(device=dev).manual_seed(11 + size)
        sets = torch.rand((nq, nl), generator=gen, device=dev).argsort(1)[:, :size].contiguous()  # distinct labels per query
        first = (torch.arange(nq + 1, device=dev) * size).to(torch.int32)
        values = sets.reshape(-1).to(torch.int32)
        per_query = table[sets[:, 0]].clone()  # [nq, nw]: the union, what the scan needs
        for j in range(1, size):
            per_query |= table[sets[:, j]]
        want = sets[:, 0].to(torch.int32).contiguous()
        torch.cuda.synchronize()

        def labelset():
            ids, d, ln, st = out["labelset"]
            index.search_exact_labelset_device(labels, nq, nq * size, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                                               st.data_ptr(), queries=qrows.data_ptr(), ldq=ld, want_first=first.data_ptr(),
                                               want_values=values.data_ptr(), stream=stream.cuda_stream)

        def scan():
            ids, d, ln, st = out["scan"]
            index.search_exact_filtered_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                               queries=qrows.data_ptr(), ldq=ld, allow=per_query.data_ptr(), allow_stride=nw,
                                               stream=stream.cuda_stream)

        def labeled():
            ids, d, ln, st = out["labeled"]
            index.search_exact_labeled_device(labels, nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), st.data_ptr(),
                                              queries=qrows.data_ptr(), ldq=ld, want=want.data_ptr(), stream=stream.cuda_stream)

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

        variants = [("labelset", labelset), ("scan", scan)] + ([("labeled", labeled)] if size == 1 else [])
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for v, f in variants:
                runs[v].append(timed(v, f))
        rows = {v: [x.cpu().numpy() for x in out[v][:3]] for v, _ in variants}

        def rows_equal(x, y):
            return bool((x[0] == y[0]).all() and (x[1].view(np.uint32) == y[1].view(np.uint32)).all() and (x[2] == y[2]).all())

        line = {"set_size": size, "labels": nl, "rows_per_label": each, "vectors": n, "dim": dim, "queries": nq, "k": k,
                "pairs": nq * size, "candidates_per_query": size * each, "steps": args.steps, "warmup": args.warmup,
                "rounds": args.runs}
        for v, _ in variants:
            med = float(np.median(runs[v]))
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": med, "spread": round(max(runs[v]) - min(runs[v]), 4)}
            if v != "labelset":
                line["labelset_rows_equal_%s_rows" % v] = rows_equal(rows["labelset"], rows[v])
                line["%s_over_labelset" % v] = round(med / line["labelset_ms_per_step"]["median"], 3)
        print(json.dumps(line), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        assert all(line["labelset_rows_equal_%s_rows" % v] for v, _ in variants[1:]), "rows differ at %s" % cell
        del per_query


if __name__ == "__main__":
    main()
