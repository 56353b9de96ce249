"""The exact radius search (phnsw_search_exact_radius_device) beside the exact top-k over the same tables
(phnsw_search_exact_shared_device, no filter, k = 10) on the bench.py workload: the 1M x 768 clustered "survey" set, the
same seeds, 10 000-query batches, device-resident, one stream.  Neither call walks the graph, so the index is an adopted
one-layer ring (no build).  One cell per radius level: ONE radius for the batch, chosen so that the mean number of rows
inside it is about 10, 100 and 1000.

The radii do not come from the code under test: the distances of a sample of the queries to every row are computed by
brute force in torch ((1 - cos) / 2 in float32), and the radius of a level is the value that many of the sample's
distances lie below.  What the whole batch then finds inside it is reported per cell (`in_radius_mean`, `in_radius_max`).

Per cell the variants -- `radius` (cap = the total, known from a first call), `count` (cap 0: no record kept or sorted)
and `topk` -- are timed ALTERNATELY inside this one run, --runs rounds, each round --warmup + --steps launches per variant
between two device events; median and spread (max - min) of the rounds' ms per step are reported.  `topk` shares the
table work, so `radius - topk` is what compaction, sort and unpack cost beside the top-k select.  All three synchronise
their stream by contract (radius twice, the others once); those waits are inside their times.  The steps of `radius`
(count, list, pack + table, compact, scan + sort) come from the library's own events: one extra call per cell with
PHNSW_DENSE_TIMES=1.  The unpack is enqueued after the call's last event and is in the step time only.

With --walk the index is built (ph.Hnsw.generate, the benchmark's build) and the radius search by graph walk
(phnsw_search_batch_radius_device, max_out 1024) is measured per radius level and per number_of_candidates in --efs,
upper_layer_candidate_count = number_of_candidates / 4 (a bottom-layer queue that starts full cannot grow: with the two
equal the loop ends after one call), probe_depth 2: its time against the plain walk at the same parameters
(phnsw_search_batch_device, the device form of phnsw_search_batch_topk's search), alternating as above; the share of the
exact in-radius rows (phnsw_search_exact_radius_device's segments) that the walk returns; the share of queries with
status 6; the share with out_len above max_out.

  python scripts/radius_profile.py [--levels 10,100,1000] [--walk] [--efs 128,256,512] [--out FILE] [--readme FILE]"""
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


def brute_force_radii(torch, rows, queries, levels, sample):
    """per level the f32 value below which sample * level of the sample's distances lie; rows, queries: device tensors"""
    q = queries[torch.linspace(0, len(queries) - 1, sample, device=queries.device).long()]
    q = q / q.norm(dim=1, keepdim=True)
    most = int(sample * max(levels)) + 1
    best = None
    for at in range(0, len(rows), 1 << 17):  # the smallest `most` distances, kept over row blocks
        r = rows[at:at + (1 << 17)]
        d = ((1.0 - q @ (r / r.norm(dim=1, keepdim=True)).T) * 0.5).flatten()
        best = d if best is None else torch.cat([best, d])
        if len(best) > most:
            best = torch.topk(best, most, largest=False).values
    best = torch.sort(best).values
    return [float(best[int(sample * level)].item()) for level in levels]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="10,100,1000", help="mean rows inside the radius, per cell")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--sample", type=int, default=500, help="queries the brute-force radii are taken from")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5, help="rounds, the variants alternating inside each")
    ap.add_argument("--walk", action="store_true", help="build the index and measure the radius walk too")
    ap.add_argument("--efs", default="128,256,512", help="number_of_candidates of the walk's cells")
    ap.add_argument("--out", default="")
    ap.add_argument("--readme", default="", help="write the cells as a markdown table here")
    args = ap.parse_args()
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, args.k
    levels = [float(x) for x in args.levels.split(",")]
    noise = 0.1 * dim ** 0.5
    full = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    ring = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + n - 1) % n], axis=1).astype(np.uint64)
    if args.walk:
        index = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters())
    else:
        index = ph.Hnsw.from_layers(full, [(np.arange(n, dtype=np.uint64), ring)])
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    rows_t = torch.from_numpy(full.read()[:, :dim]).to(dev)
    q_t = torch.from_numpy(qs.read()[:, :dim]).to(dev)
    radii = brute_force_radii(torch, rows_t, q_t, levels, min(args.sample, nq))
    del rows_t, q_t
    torch.cuda.empty_cache()

    stream = torch.cuda.Stream()
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    first = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    t_ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    t_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    t_ln = torch.empty(nq, dtype=torch.int32, device=dev)
    lines = []
    for level, r in zip(levels, radii):
        rad = torch.full((nq,), r, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def count():
            index.search_exact_radius_device(nq, rad.data_ptr(), 0, first.data_ptr(), 0, 0, status.data_ptr(), total.data_ptr(),
                                             queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream)

        count()
        torch.cuda.synchronize()
        found = int(total.cpu().numpy()[0])
        per_query = np.diff(first.cpu().numpy())
        cap = max(found, 1)
        ids = torch.empty(cap, dtype=torch.int32, device=dev)
        d = torch.empty(cap, dtype=torch.float32, device=dev)

        def radius():
            index.search_exact_radius_device(nq, rad.data_ptr(), cap, first.data_ptr(), ids.data_ptr(), d.data_ptr(),
                                             status.data_ptr(), total.data_ptr(), queries=qs.rows_dev, ldq=qs.ld,
                                             stream=stream.cuda_stream)

        def topk():
            index.search_exact_shared_device(nq, k, t_ids.data_ptr(), t_d.data_ptr(), t_ln.data_ptr(), status.data_ptr(),
                                             queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream)

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

        variants = (("radius", radius), ("count", count), ("topk", topk))
        runs = {v: [] for v, _ in variants}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all three
            for v, f in variants:
                runs[v].append(timed(f))
        # the rows inside the radius against the top-k's: the leading min(k, count) of every segment are its row
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
        m = re.search(r"count ([\d.]+) ms, list ([\d.]+) ms, pack\+table ([\d.]+) ms, compact ([\d.]+) ms, scan\+sort ([\d.]+) ms", text)
        steps = dict(zip(("count", "list", "pack_table", "compact", "scan_sort"), map(float, m.groups()))) if m else None
        line = {"level": level, "radius": r, "vectors": n, "dim": dim, "queries": nq, "k": k, "in_radius_total": found,
                "in_radius_mean": round(found / nq, 2), "in_radius_max": int(per_query.max()),
                "queries_with_none": int((per_query == 0).sum()), "steps": args.steps, "warmup": args.warmup, "rounds": args.runs,
                "leading_rows_equal_topk": bool(agree), "radius_steps_ms": steps}
        for v, _ in variants:
            line[v + "_ms_per_step"] = {"rounds": runs[v], "median": float(np.median(runs[v])),
                                        "spread": round(max(runs[v]) - min(runs[v]), 4)}
        line["radius_minus_topk_ms"] = round(line["radius_ms_per_step"]["median"] - line["topk_ms_per_step"]["median"], 4)
        line["radius_over_topk"] = round(line["radius_ms_per_step"]["median"] / line["topk_ms_per_step"]["median"], 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
        assert agree, "the radius call and the top-k disagree at level %g" % level
        if args.walk:
            line["walk"] = walk_cells(torch, ph, index, qs, rad, (f_h, i_h), [int(x) for x in args.efs.split(",")], args, stream, timed)
            print(json.dumps({"level": level, "walk": line["walk"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    if args.readme:
        os.makedirs(os.path.dirname(os.path.abspath(args.readme)), exist_ok=True)
        with open(args.readme, "w") as f:
            f.write(readme(lines, args))


def walk_cells(torch, ph, index, qs, rad, exact, efs, args, stream, timed):
    """one cell per number_of_candidates: the radius walk beside the plain walk, and what it finds of the exact segments"""
    dev = torch.device("cuda:0")
    nq, max_out = len(rad), 1024
    f_h, i_h = exact
    ids = torch.empty((nq, max_out), dtype=torch.int32, device=dev)
    d = torch.empty((nq, max_out), dtype=torch.float32, device=dev)
    ln = torch.empty(nq, dtype=torch.int32, device=dev)
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    cells = []
    for ef in efs:
        sp = ph.SearchParameters(ef, max(ef // 4, 1), 2)
        p_ids = torch.empty((nq, ef), dtype=torch.int32, device=dev)
        p_d = torch.empty((nq, ef), dtype=torch.float32, device=dev)
        p_ln = torch.empty(nq, dtype=torch.int32, device=dev)
        p_status = torch.zeros(nq, dtype=torch.int32, device=dev)

        def walk():
            index.search_radius_device(nq, sp, rad.data_ptr(), max_out, ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                                       status.data_ptr(), queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream)

        def plain():
            index.search_batch_device(nq, sp, p_ids.data_ptr(), p_d.data_ptr(), p_ln.data_ptr(), p_status.data_ptr(),
                                      queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream)

        def timed_any(launch):  # `timed` asserts a clean status: the walk's status 6 is a figure here, not a failure
            for _ in range(args.warmup):
                launch()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.steps):
                launch()
            b.record(stream)
            torch.cuda.synchronize()
            return round(a.elapsed_time(b) / args.steps, 4)

        runs = {"walk": [], "plain": []}
        for _ in range(args.runs):
            runs["walk"].append(timed_any(walk))
            runs["plain"].append(timed_any(plain))
        st = status.cpu().numpy()
        wl = ln.cpu().numpy().astype(np.int64)
        wi = ids.cpu().numpy()
        assert not p_status.cpu().numpy().any() and not ((st != 0) & (st != 6)).any()
        hit = sum(len(np.intersect1d(wi[i, :min(wl[i], max_out)], i_h[f_h[i]:f_h[i + 1]], assume_unique=True)) for i in range(nq))
        cell = {"number_of_candidates": ef, "upper_layer_candidate_count": max(ef // 4, 1), "probe_depth": 2, "max_out": max_out,
                "share_of_exact_rows_returned": round(hit / max(int(f_h[nq]), 1), 4), "status_6_share": round(float((st == 6).mean()), 4),
                "out_len_above_max_out_share": round(float((wl > max_out).mean()), 4), "out_len_mean": round(float(wl.mean()), 2)}
        for v in ("walk", "plain"):
            cell[v + "_ms_per_step"] = {"rounds": runs[v], "median": float(np.median(runs[v])), "spread": round(max(runs[v]) - min(runs[v]), 4)}
        cell["walk_over_plain"] = round(cell["walk_ms_per_step"]["median"] / cell["plain_ms_per_step"]["median"], 3)
        cells.append(cell)
    return cells


def readme(lines, args):
    ms = lambda x: "%.2f (%.2f)" % (x["median"], x["spread"])
    out = ["# Exact radius search: what it costs beside the exact top-k", "",
           "Written by `scripts/radius_profile.py` (its docstring has the method): %d x %d f32 rows, the benchmark's clustered set,"
           % (lines[0]["vectors"], lines[0]["dim"]),
           "cosine, %d queries a batch, no filter (every row is a candidate), one MI355X.  Times are ms per call, the median of %d"
           % (lines[0]["queries"], args.runs),
           "rounds with the spread (max - min) in brackets; the three calls alternate inside a round.", "",
           "| rows inside the radius, mean (max) | radius | count only | top-k, k = %d | radius - top-k | table | compact | scan + sort |" % lines[0]["k"],
           "|---|---|---|---|---|---|---|---|"]
    for x in lines:
        s = x["radius_steps_ms"] or {}
        out.append("| %.1f (%d) | %s | %s | %s | %.2f | %s | %s | %s |" % (
            x["in_radius_mean"], x["in_radius_max"], ms(x["radius_ms_per_step"]), ms(x["count_ms_per_step"]), ms(x["topk_ms_per_step"]),
            x["radius_minus_topk_ms"], s.get("pack_table", "-"), s.get("compact", "-"), s.get("scan_sort", "-")))
    if any("walk" in x for x in lines):
        out += ["", "## The radius search by graph walk", "",
                "`phnsw_search_batch_radius_device`, max_out 1024, upper_layer_candidate_count = number_of_candidates / 4, probe_depth 2,",
                "against the plain walk at the same parameters (`phnsw_search_batch_device`); the built index.  `found` is the share of the",
                "exact in-radius rows that the walk returned (over all queries, those with status 6 returning none).", "",
                "| rows inside the radius, mean | number_of_candidates | radius walk | plain walk | ratio | found | status 6 | out_len > max_out |",
                "|---|---|---|---|---|---|---|---|"]
        for x in lines:
            for c in x.get("walk", []):
                out.append("| %.1f | %d | %s | %s | %.2f | %.4f | %.4f | %.4f |" % (
                    x["in_radius_mean"], c["number_of_candidates"], ms(c["walk_ms_per_step"]), ms(c["plain_ms_per_step"]),
                    c["walk_over_plain"], c["share_of_exact_rows_returned"], c["status_6_share"], c["out_len_above_max_out_share"]))
    out += ["", "The leading min(k, count) entries of every segment equalled the top-k's row in ids and distance bits in every cell: %s."
            % all(x["leading_rows_equal_topk"] for x in lines),
            "Not measured: f16, i8 and i8q stores, L2 and ragged dimensions (the vector-unit pass), a filter, per-query radii,",
            "other batch sizes, the host form, a cap below the total (two calls)."]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
