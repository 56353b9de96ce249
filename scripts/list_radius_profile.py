"""The exact radius search by row label and by numeric range (phnsw_search_exact_radius_labeled_device, _ranged_device)
beside the calls that read the same rows and the call it replaces, on the bench.py workload: the 1M x 768 clustered
"survey" set, the same seeds, 10 000-query batches, device-resident, one stream.  No call walks the graph, so the index is
an adopted one-layer ring (no build).

Cells: lists of --lengths rows (labels: 8 labels of 100 000 rows, 64 of 10 000, else n / length labels, label of row v =
v % labels below labels * length and none above, query i wants label i % labels; ranges: key of row v = (v * 7919) % n,
a bijection, query i takes the window of `length` keys that starts at (i * 104729) % (n - length)), times --levels, the
mean number of rows inside the radius.  ONE radius per cell: the
distances of a sample of the queries to the rows of their own list are computed by brute force in torch ((1 - cos) / 2
in float32), and the radius is the value that many of them lie below.  Nothing of it comes from the code under test.

Per cell, timed ALTERNATELY inside one run (--runs rounds of --warmup + --steps launches between two device events;
median and spread of the rounds' ms per step):
  radius   cap = the total, known from a first call
  count    cap 0: no record kept or sorted
  topk     phnsw_search_exact_labeled_device under PHNSW_LABEL_TILE=1 / phnsw_search_exact_ranged_device at k = 10: the
           per-query top-k scan over the same lists, which reads the same rows
  bitmap   (labels only, --bitmap) phnsw_search_exact_radius_device once per distinct label with its bitmap and the
           queries that want it, one step = all those calls: what a caller had to do before.  Warmed and timed in the
           same rounds as the others
The scan kernel alone and scan + sort come from the library's own events: one extra call per cell with PHNSW_DENSE_TIMES=1.

  python scripts/list_radius_profile.py [--lengths 100000,10000,1000] [--levels 10,100,1000] [--bitmap] [--out FILE] [--readme FILE]"""
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


def radius_of(torch, rows, queries, lists, level):
    """the f32 value below which len(lists) * level of the distances of sample query j to the rows lists[j] lie"""
    best = []
    for q, ids in zip(queries, lists):
        r = rows[ids]
        d = (1.0 - (r / r.norm(dim=1, keepdim=True)) @ (q / q.norm())) * 0.5
        best.append(torch.topk(d, min(len(d), int(8 * level) + 8), largest=False).values)
    best = torch.sort(torch.cat(best)).values
    return float(best[min(int(len(lists) * level), len(best) - 1)].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="100000,10000,1000")
    ap.add_argument("--levels", default="10,100,1000", help="mean rows inside the radius, per cell")
    ap.add_argument("--kinds", default="labeled,ranged")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bitmap", action="store_true", help="also the shared-bitmap radius call, once per distinct label")
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="")
    args = ap.parse_args()
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, args.k
    noise = 0.1 * dim ** 0.5
    full = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    ring = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + n - 1) % n], axis=1).astype(np.uint64)
    index = ph.Hnsw.from_layers(full, [(np.arange(n, dtype=np.uint64), ring)])
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    rows_t = torch.from_numpy(full.read()[:, :dim]).to(dev)
    q_t = torch.from_numpy(qs.read()[:, :dim]).to(dev)
    sample = np.linspace(0, nq - 1, min(args.sample, nq)).astype(np.int64)
    keys = (np.arange(n, dtype=np.uint64) * 7919 % n).astype(np.uint32)
    by_key = np.argsort(keys, kind="stable")
    attr = ph.Attribute(index, keys) if "ranged" in args.kinds else None

    stream = torch.cuda.Stream()
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    first = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    t_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    t_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    t_ln = torch.empty(nq, dtype=torch.int32, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    lines = []
    for kind in args.kinds.split(","):
        for length in [int(x) for x in args.lengths.split(",")]:
            if kind == "labeled":
                nlabels = min(n // length, {100000: 8, 10000: 64}.get(length, n // length))
                lab = (np.arange(n) % nlabels).astype(np.uint32)
                lab[nlabels * length:] = 0xFFFFFFFF  # the rows past the last full list carry no label
                want = (np.arange(nq) % nlabels).astype(np.uint32)
                handle = ph.Labels(index, lab)
                want_t = up(want)
                filt = dict(want=want_t.data_ptr())
                lists = [torch.arange(int(want[i]), nlabels * length, nlabels, device=dev) for i in sample]
            else:
                lo = (np.arange(nq, dtype=np.uint64) * 104729 % (n - length)).astype(np.uint32)
                hi = lo + np.uint32(length - 1)
                handle = attr
                lo_t, hi_t = up(lo), up(hi)
                filt = dict(lo=lo_t.data_ptr(), hi=hi_t.data_ptr())
                lists = [torch.from_numpy(by_key[int(lo[i]):int(hi[i]) + 1]).to(dev) for i in sample]
            call = getattr(index, "search_exact_radius_%s_device" % kind)
            top = getattr(index, "search_exact_%s_device" % kind)
            for level in [float(x) for x in args.levels.split(",")]:
                r = radius_of(torch, rows_t, q_t[torch.from_numpy(sample).to(dev)], lists, level)
                rad = torch.full((nq,), r, dtype=torch.float32, device=dev)
                torch.cuda.synchronize()

                def count():
                    call(handle, nq, rad.data_ptr(), 0, first.data_ptr(), 0, 0, status.data_ptr(), total.data_ptr(),
                         queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream, **filt)

                count()
                torch.cuda.synchronize()
                found = int(total.cpu().numpy()[0])
                per_query = np.diff(first.cpu().numpy())
                cap = max(found, 1)
                ids = torch.empty(cap, dtype=torch.int32, device=dev)
                d = torch.empty(cap, dtype=torch.float32, device=dev)

                def radius():
                    call(handle, nq, rad.data_ptr(), cap, first.data_ptr(), ids.data_ptr(), d.data_ptr(), status.data_ptr(),
                         total.data_ptr(), queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream, **filt)

                def topk():
                    os.environ["PHNSW_LABEL_TILE"] = "1"  # the per-query path: the rows this call reads, read the same way
                    try:
                        top(handle, nq, k, t_ids.data_ptr(), t_d.data_ptr(), t_ln.data_ptr(), status.data_ptr(), queries=qs.rows_dev,
                            ldq=qs.ld, stream=stream.cuda_stream, **filt)
                    finally:
                        del os.environ["PHNSW_LABEL_TILE"]

                def timed(launch, steps=args.steps, warmup=args.warmup):
                    for _ in range(warmup):
                        launch()
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for _ in range(steps):
                        launch()
                    b.record(stream)
                    torch.cuda.synchronize()
                    assert not status.cpu().numpy().any(), "a query failed"
                    return round(a.elapsed_time(b) / steps, 4)

                variants = [("radius", radius), ("count", count), ("topk", topk)]
                if args.bitmap and kind == "labeled":
                    groups = [np.nonzero(want == l)[0] for l in range(nlabels)]
                    words = [up(ph.hnsw.pack_allow(lab == l, n, 1)[0]) for l in range(nlabels)]
                    q_h = qs.read()
                    sub = [(torch.from_numpy(q_h[g]).to(dev), torch.full((len(g),), r, dtype=torch.float32, device=dev)) for g in groups]
                    b_first = torch.empty(nq + 1, dtype=torch.int64, device=dev)  # outputs of its own: the radius call's stay
                    b_ids = torch.empty(cap, dtype=torch.int32, device=dev)
                    b_d = torch.empty(cap, dtype=torch.float32, device=dev)
                    b_total = torch.zeros(1, dtype=torch.int64, device=dev)

                    def bitmap():
                        for (qd, rd), w, g in zip(sub, words, groups):
                            index.search_exact_radius_device(len(g), rd.data_ptr(), cap, b_first.data_ptr(), b_ids.data_ptr(),
                                                             b_d.data_ptr(), status.data_ptr(), b_total.data_ptr(), queries=qd.data_ptr(),
                                                             ldq=qs.ld, allow=w.data_ptr(), stream=stream.cuda_stream)
                    variants.append(("bitmap", bitmap))
                runs = {v: [] for v, _ in variants}
                for _ in range(args.runs):  # alternating: a drift of the machine lands on all
                    for v, f in variants:
                        runs[v].append(timed(f))
                f_h, i_h, d_h = first.cpu().numpy(), ids.cpu().numpy(), d.cpu().numpy()
                ti, td = t_ids.cpu().numpy(), t_d.cpu().numpy()
                agree = all((i_h[f_h[i]:f_h[i] + min(k, per_query[i])] == ti[i, :min(k, per_query[i])]).all() and
                            (d_h[f_h[i]:f_h[i] + min(k, per_query[i])].view(np.uint32) == td[i, :min(k, per_query[i])].view(np.uint32)).all()
                            for i in range(nq))
                os.environ["PHNSW_DENSE_TIMES"] = "1"
                try:
                    text = captured_stderr(lambda: (radius(), torch.cuda.synchronize()))
                finally:
                    del os.environ["PHNSW_DENSE_TIMES"]
                m = re.search(r"in (\d+) slices.*lookup ([\d.]+) ms, scan ([\d.]+) ms, scan\+sort ([\d.]+) ms", text)
                line = {"kind": kind, "list_rows": length, "level": level, "radius": r, "vectors": n, "dim": dim, "queries": nq, "k": k,
                        "in_radius_total": found, "in_radius_mean": round(found / nq, 2), "in_radius_max": int(per_query.max()),
                        "steps": args.steps, "warmup": args.warmup, "rounds": args.runs, "leading_rows_equal_topk": bool(agree),
                        "slices": int(m.group(1)) if m else None, "lookup_ms": float(m.group(2)) if m else None,
                        "scan_ms": float(m.group(3)) if m else None, "scan_sort_ms": float(m.group(4)) if m else None}
                if args.bitmap and kind == "labeled":
                    line["bitmap_calls"] = nlabels
                for v, _ in variants:
                    line[v + "_ms_per_step"] = {"rounds": runs[v], "median": float(np.median(runs[v])),
                                                "spread": round(max(runs[v]) - min(runs[v]), 4)}
                line["radius_minus_topk_ms"] = round(line["radius_ms_per_step"]["median"] - line["topk_ms_per_step"]["median"], 4)
                line["radius_over_topk"] = round(line["radius_ms_per_step"]["median"] / line["topk_ms_per_step"]["median"], 3)
                print(json.dumps(line), flush=True)
                lines.append(line)
                assert agree, "the radius call and the top-k disagree (%s, %d rows, level %g)" % (kind, length, level)
            if kind == "labeled":
                handle.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    if args.readme:
        os.makedirs(os.path.dirname(os.path.abspath(args.readme)), exist_ok=True)
        with open(args.readme, "w") as f:
            f.write(readme(lines, args))


def readme(lines, args):
    ms = lambda x: "%.2f (%.2f)" % (x["median"], x["spread"])
    out = ["# Exact radius search by row label and by numeric range: what it costs", "",
           "Written by `scripts/list_radius_profile.py` (its docstring has the method): %d x %d f32 rows, the benchmark's clustered"
           % (lines[0]["vectors"], lines[0]["dim"]),
           "set, cosine, %d queries a batch, one MI355X.  Times are ms per call, the median of %d rounds with the spread (max - min)"
           % (lines[0]["queries"], args.runs),
           "in brackets; the calls alternate inside a round.  `top-k` is the per-query top-k scan over the same lists at k = %d"
           % lines[0]["k"],
           "(`phnsw_search_exact_labeled` under `PHNSW_LABEL_TILE=1`, `phnsw_search_exact_ranged`); `bitmap` is",
           "`phnsw_search_exact_radius` called once per distinct label with its bitmap, one step being all those calls.", "",
           "| filter | rows per list | rows inside the radius, mean (max) | radius | count only | top-k | radius - top-k | slices | scan kernel | scan + sort | bitmap calls |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for x in lines:
        b = x.get("bitmap_ms_per_step")
        out.append("| %s | %d | %.1f (%d) | %s | %s | %s | %.2f | %s | %s | %s | %s |" % (
            x["kind"], x["list_rows"], x["in_radius_mean"], x["in_radius_max"], ms(x["radius_ms_per_step"]), ms(x["count_ms_per_step"]),
            ms(x["topk_ms_per_step"]), x["radius_minus_topk_ms"], x["slices"], x["scan_ms"], x["scan_sort_ms"],
            "%s, %d calls" % (ms(b), x["bitmap_calls"]) if b else "-"))
    out += ["", "The leading min(k, count) entries of every segment equalled the top-k's row in ids and distance bits in every cell: %s."
            % all(x["leading_rows_equal_topk"] for x in lines)]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
