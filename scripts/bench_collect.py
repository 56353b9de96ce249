"""The collecting walk (phnsw_search_collect_device, phnsw_search_collect_labeled_device) beside what a filtered-search
user had before it, on the bench.py workload: the 1M x 768 clustered f32 rows (the same seeds and build), 10 000
device-resident queries, ef 256 / probe_depth 8, k = 10, one stream.

Cells: densities 0.5 %, 1 %, 2 %, 5 %, 20 %, each as ONE SHARED BITMAP and BY LABEL (a label column in which label 0 has
that density; every query wants label 0).  Per cell, the calls ALTERNATING in every round:

  plain           phnsw_search_batch_device: no filter at all -- the descent a collecting search runs, as the time to hold
                  collect against (its rows are not results of the cell: no recall is reported for it)
  strict          phnsw_search_batch_filtered_device / phnsw_search_batch_labeled_device, PHNSW_FILTER_STRICT: the post-filter
  auto            phnsw_search_filtered_auto_device / phnsw_search_labeled_auto_device, the library's scan_below
  collect         phnsw_search_collect[_labeled]_device, flags 0
  collect_extend  ... with PHNSW_COLLECT_EXTEND

and per call: ms per batch from device events after warm-up (median of --runs rounds and their spread), results per query
(cut to k), recall@k against phnsw_search_exact_filtered_device / phnsw_search_exact_labeled_device (the share of the
exact row's ids a row holds, averaged over the queries whose exact row is not empty), and the evaluations per query of the
walks that report them.  One JSON line per cell and call.

  python scripts/bench_collect.py [--densities ...] [--forms shared,label] [--index-file FILE] [--out FILE]

The filtered walk of ANOTHER CHECKOUT (the parent commit, built in its own tree) against this one, alternating:

  python scripts/bench_collect.py --walk-only --package-root DIR      one process: plain, the strict walk (and, where the
                                                                      checkout has it, collect without EXTEND) per cell
  python scripts/bench_collect.py --ab DIR --ab-rounds 3 --index-file FILE
      spawns those processes in turn -- DIR, this checkout, DIR, ... -- over one serialised index and prints, per cell, the
      strict walk's and the plain search's ms in either checkout, the run-to-run spread of each, and collect (flags 0) over
      the parent's strict walk and over the parent's plain search.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--densities", default="0.005,0.01,0.02,0.05,0.2")
    ap.add_argument("--forms", default="shared,label")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=256)
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="rounds of every timed measurement, the calls alternating")
    ap.add_argument("--index-file", default="", help="load the index from here if the file exists, else build and save it")
    ap.add_argument("--package-root", default=HERE, help="the checkout whose parallel_hnsw_amd is imported")
    ap.add_argument("--walk-only", action="store_true", help="time the strict walk (and collect, if present) only")
    ap.add_argument("--ab", default="", help="another checkout (built): alternate --walk-only processes of it and of this one")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    return ap.parse_args()


def emit(args, lines):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def ab(args):
    """alternating child processes; every child prints one JSON line per cell and call"""
    got = {}
    order = []
    for r in range(args.ab_rounds):
        for tag, root in (("parent", args.ab), ("this", HERE)):
            cmd = [sys.executable, os.path.abspath(__file__), "--walk-only", "--package-root", root]
            for name in ("densities", "forms", "n", "dim", "nq", "k", "ef", "probe_depth", "steps", "warmup", "runs", "index_file"):
                flag = {"n": "--vectors", "nq": "--queries"}.get(name, "--" + name.replace("_", "-"))
                if getattr(args, name) != "":
                    cmd += [flag, str(getattr(args, name))]
            env = dict(os.environ)
            env.pop("PHNSW_LIB_PATH", None)
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    j = json.loads(line)
                    key = (j["form"], j["density"], tag, j["call"])
                    got.setdefault(key, []).append(j["ms_per_batch"]["median"])
                    if (j["form"], j["density"]) not in order:
                        order.append((j["form"], j["density"]))
    lines = []
    for form, dens in order:
        p, t, c, pp, tp = (got.get((form, dens, tag, call), []) for tag, call in
                           (("parent", "strict"), ("this", "strict"), ("this", "collect"), ("parent", "plain"), ("this", "plain")))
        line = {"ab": True, "form": form, "density": dens, "rounds": args.ab_rounds,
                "parent_strict_ms": p, "this_strict_ms": t, "this_collect_ms": c,
                "parent_spread": round(max(p) - min(p), 4), "this_spread": round(max(t) - min(t), 4),
                "strict_this_over_parent": round(float(np.median(t) / np.median(p)), 4),
                "collect_over_parent_strict": round(float(np.median(c) / np.median(p)), 4) if c else None,
                "parent_plain_ms": pp, "this_plain_ms": tp, "parent_plain_spread": round(max(pp) - min(pp), 4),
                "plain_this_over_parent": round(float(np.median(tp) / np.median(pp)), 4),
                "collect_over_parent_plain": round(float(np.median(c) / np.median(pp)), 4) if c else None}
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    emit(args, lines)


def main():
    args = parse()
    if args.ab:
        return ab(args)
    sys.path.insert(0, args.package_root)
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, args.k
    has_collect = hasattr(ph.Hnsw, "search_collect_device")
    noise = 0.1 * dim ** 0.5
    store = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    if args.index_file and os.path.exists(args.index_file):
        index = ph.Hnsw.deserialize(args.index_file, store)
    else:
        index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
        if args.index_file:
            index.serialize(args.index_file)
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    stream = torch.cuda.Stream()
    sp = ph.SearchParameters(args.ef, args.ef, args.probe_depth)
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    lines = []

    def rows(width):
        return (torch.empty((nq, width), dtype=torch.int32, device=dev), torch.empty((nq, width), dtype=torch.float32, device=dev),
                torch.empty(nq, dtype=torch.int32, device=dev), torch.zeros((nq, 2), dtype=torch.int32, device=dev))

    for form in args.forms.split(","):
        for dens in (float(x) for x in args.densities.split(",")):
            allowed = torch.rand(n, generator=torch.Generator(device=dev).manual_seed(7), device=dev) < dens
            common = dict(queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream)
            if form == "shared":
                a = allowed.cpu().numpy()
                words = torch.from_numpy(ph.hnsw.pack_allow(a, n, nq)[0].view(np.int32)).to(dev)
                filt = dict(allow=words.data_ptr(), allow_stride=0)

                def exact(o):
                    index.search_exact_filtered_device(nq, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), status.data_ptr(),
                                                       **filt, **common)

                def strict(o):
                    index.search_batch_filtered_device(nq, sp, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), status.data_ptr(),
                                                       strict=True, out_stats=o[3].data_ptr(), **filt, **common)

                def auto(o):
                    index.search_filtered_device(nq, sp, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), status.data_ptr(),
                                                 **filt, **common)

                def collect(o, extend=False, width=k):
                    index.search_collect_device(nq, sp, width, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), status.data_ptr(),
                                                extend=extend, out_stats=o[3].data_ptr(), **filt, **common)
            else:
                lab = np.where(allowed.cpu().numpy(), 0, 1)
                labels = ph.Labels(index, lab)
                want = torch.zeros(nq, dtype=torch.int32, device=dev)
                filt = dict(want=want.data_ptr())

                def exact(o):
                    index.search_exact_labeled_device(labels, nq, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                      status.data_ptr(), **filt, **common)

                def strict(o):
                    index.search_batch_labeled_device(labels, nq, sp, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                      status.data_ptr(), strict=True, out_stats=o[3].data_ptr(), **filt, **common)

                def auto(o):
                    index.search_labeled_device(labels, nq, sp, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                status.data_ptr(), **filt, **common)

                def collect(o, extend=False, width=k):
                    index.search_collect_labeled_device(labels, nq, sp, width, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                        status.data_ptr(), extend=extend, out_stats=o[3].data_ptr(), **filt, **common)

            def plain(o):  # the unfiltered search: the descent a collecting search runs
                index.search_batch_device(nq, sp, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), status.data_ptr(),
                                          out_stats=o[3].data_ptr(), **common)

            calls = [("plain", plain, rows(args.ef)), ("strict", strict, rows(args.ef))]
            if not args.walk_only:
                calls.append(("auto", auto, rows(k)))
            if has_collect:
                calls.append(("collect", collect, rows(k)))
                if not args.walk_only:
                    calls.append(("collect_extend", lambda o: collect(o, True), rows(k)))

            def timed(f, o):
                for _ in range(args.warmup):
                    f(o)
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(args.steps):
                    f(o)
                t1.record(stream)
                torch.cuda.synchronize()
                assert not status.cpu().numpy().any(), "a query failed"
                return round(t0.elapsed_time(t1) / args.steps, 4)

            runs = {name: [] for name, _, _ in calls}
            for _ in range(args.runs):  # alternating: a drift of the machine lands on every call
                for name, f, o in calls:
                    runs[name].append(timed(f, o))
            wide = None
            if has_collect and not args.walk_only:  # the walk's yield past k: one untimed call with the widest `kept`
                w = (torch.empty((nq, 64), dtype=torch.int32, device=dev), torch.empty((nq, 64), dtype=torch.float32, device=dev),
                     torch.empty(nq, dtype=torch.int32, device=dev), torch.zeros((nq, 2), dtype=torch.int32, device=dev))
                collect(w, width=64)
                torch.cuda.synchronize()
                wide = round(float(w[2].cpu().numpy().astype(np.int64).mean()), 3)
            truth = None
            if not args.walk_only:
                truth = rows(k)
                exact(truth)
                torch.cuda.synchronize()
                t_ids, t_len = truth[0].cpu().numpy().view(np.uint32), truth[2].cpu().numpy().astype(np.int64)
            for name, f, o in calls:
                r = runs[name]
                ids = o[0].cpu().numpy().view(np.uint32)[:, :k]
                ln = np.minimum(o[2].cpu().numpy().astype(np.int64), k)
                line = {"form": form, "density": dens, "call": name, "vectors": n, "dim": dim, "queries": nq, "k": k, "ef": args.ef,
                        "probe_depth": args.probe_depth, "allowed_rows": int(allowed.sum().item()), "steps": args.steps,
                        "warmup": args.warmup,
                        "ms_per_batch": {"runs": r, "median": float(np.median(r)), "spread": round(max(r) - min(r), 4)},
                        "results_per_query": round(float(ln.mean()), 3), "rows_with_k": int((ln >= k).sum())}
                if name == "strict":  # the post-filter's whole row, before the cut to k
                    line["results_per_query_uncut"] = round(float(o[2].cpu().numpy().astype(np.int64).mean()), 3)
                if name == "collect" and wide is not None:
                    line["results_per_query_at_k64"] = wide
                if name != "auto":
                    st = o[3].cpu().numpy().view(np.uint32).astype(np.float64)
                    line.update(evaluations_per_query=round(float(st[:, 0].mean()), 1), hops_per_query=round(float(st[:, 1].mean()), 1))
                if truth is not None and name != "plain":
                    hit = [len(set(ids[i, :ln[i]].tolist()) & set(t_ids[i, :t_len[i]].tolist())) / t_len[i]
                           for i in range(nq) if t_len[i]]
                    line["recall_at_k"] = round(float(np.mean(hit)), 4)
                print(json.dumps(line), flush=True)
                lines.append(json.dumps(line))
    emit(args, lines)


if __name__ == "__main__":
    main()
