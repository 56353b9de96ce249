"""The exhaustive int8 scan over an i8q store (phnsw_i8q_scan_topk / _search, scan_i8q.hip) beside the paths the tree
already had, on the bench.py workload: the 1M x 768 clustered "survey" set, 10 000-query batches, k = 10, one stream,
device forms, device-event times.  Appends to profiles/i8q_scan/i8q_scan_profile.jsonl (the README there is written from
it).  Nothing here is asserted anywhere: the script reports what it finds.

  python scripts/i8q_scan_profile.py [--candidates 64,256,1024] [--runs 3] [--tiles 0,32] [--no-index]
      the measurement (needs an MI355X).  Per r: ms per batch of the new scan alone, the new scan + re-rank and the fp4
      scan + re-rank, ALTERNATING inside every round (and the new scan alone again under every forced row tile of
      --tiles); recall@10 of each against the f32 brute-force top-10.  Then, with the graph (it takes minutes to build;
      --no-index leaves these out): phnsw_search_exact_shared on the i8q store with every row allowed, and the i8q
      walk + re-rank at the default search parameters.  Median and spread (max - min) of the rounds.
  python scripts/i8q_scan_profile.py --resources [--parent DIR]
      needs only hipcc: the compiler's resource report of scan_i8q.hip (resource_usage_i8q_scan.txt) and, with --parent
      pointing at the csrc directory of the parent commit, resource_usage_existing_diff.txt."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "i8q_scan")


def resources(args):
    import bits_profile as bp
    import fp4_scan_profile as fp

    fp.OUT = OUT
    os.makedirs(OUT, exist_ok=True)
    fp.resources(args)  # the fp4 unit's report and the diff of every existing unit against the parent, into OUT
    os.remove(os.path.join(OUT, "resource_usage_fp4_scan.txt"))  # profiles/fp4_scan/ has it
    mine = bp.resource_report(fp.CSRC, "scan_i8q.hip")
    with open(os.path.join(OUT, "resource_usage_i8q_scan.txt"), "w") as f:
        f.write("kernel | VGPRs | AGPRs | SGPRs | scratch bytes/lane | waves/SIMD | static LDS\n")
        for k in sorted(mine):
            r = mine[k]
            f.write("%s | %s | %s | %s | %s | %s | %s\n" % (k, r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"),
                                                        r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]"),
                                                        r.get("LDS Size [bytes/block]")))
        f.write("total: %d kernels\n" % len(mine))


def measure(args):
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, 10
    noise = 0.1 * dim ** 0.5
    make = lambda count, first: ph.VectorStore.clustered(count, dim, seed=42, first=first, n_clusters=1000, noise=noise)
    store, qs = make(n, 0), make(nq, 2 ** 32)
    i8q, fp4 = ph.I8QStore.from_full(store), ph.FP4Store.from_full(store)
    stream = torch.cuda.Stream()
    ids = torch.empty((nq, 1024), dtype=torch.int32, device=dev)
    d = torch.empty((nq, 1024), dtype=torch.float32, device=dev)
    ln = torch.empty(nq, dtype=torch.int32, device=dev)
    status = torch.zeros(nq, dtype=torch.int32, device=dev)
    o = dict(ids=ids.data_ptr(), d=d.data_ptr(), ln=ln.data_ptr(), st=status.data_ptr(), s=stream.cuda_stream)

    def timed(launch, steps, warmup):
        for _ in range(warmup):
            launch()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(steps):
            launch()
        b.record(stream)
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / steps, 4)

    def top(stride):
        return ids.cpu().numpy().reshape(-1)[: nq * stride].reshape(nq, stride)[:, :k].copy()

    def recall(fn, stride):
        fn()
        stream.synchronize()
        got = top(stride)
        return round(float(np.mean([len(set(got[i].tolist()) & set(gt[i].tolist())) / float(k) for i in range(nq)])), 4)

    def out(line):
        print(json.dumps(line), flush=True)
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "i8q_scan_profile.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")

    store.bruteforce_topk_device(qs.rows_dev, qs.ld, nq, k, o["ids"], o["d"], stream=o["s"])  # the exact f32 top-10
    stream.synchronize()
    gt = top(k)

    def forced(tile, fn):  # the knob is read per call
        def call():
            os.environ["PHNSW_I8Q_SCAN_TILE"] = str(tile)
            fn()
            os.environ.pop("PHNSW_I8Q_SCAN_TILE")
        return call

    for r in [int(x) for x in args.candidates.split(",")]:
        alone = lambda: i8q.scan_device(nq, r, qs.rows_dev, qs.ld, o["ids"], o["d"], o["ln"], stream=o["s"])
        calls = [("i8q_scan", alone, r),
                 ("i8q_scan_rerank", lambda: i8q.scan_search_device(store, nq, r, k, qs.rows_dev, qs.ld, o["ids"], o["d"], o["ln"], stream=o["s"]), r),
                 ("fp4_scan_rerank", lambda: fp4.scan_search_device(store, nq, r, k, qs.rows_dev, qs.ld, o["ids"], o["d"], o["ln"], stream=o["s"]), r)]
        calls += [("i8q_scan_tile%d" % t, forced(t, alone), r) for t in [int(x) for x in args.tiles.split(",")] if t > 0]
        runs = {name: [] for name, _, _ in calls}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for name, fn, _ in calls:
                runs[name].append(timed(fn, args.steps, args.warmup))
        out({"r": r, "vectors": n, "dim": dim, "queries": nq, "rounds": runs, "ms": {v: float(np.median(runs[v])) for v in runs},
             "spread_ms": {v: round(max(runs[v]) - min(runs[v]), 4) for v in runs},
             "recall_at_10": {name: recall(fn, stride) for name, fn, stride in calls[:3]}})
    if args.no_index:
        return
    index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
    fix = ph.Hnsw.from_layers(i8q, [(l.nodes, l.neighbors) for l in index.layers], index.build_parameters)
    allow = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)  # every row
    sp = ph.SearchParameters()
    exact = [("exact_shared_i8q", lambda: fix.search_exact_shared_device(nq, k, o["ids"], o["d"], o["ln"], o["st"], queries=qs.rows_dev,
                                                                          ldq=qs.ld, allow=allow.data_ptr(), stream=o["s"]), k),
             ("i8q_walk_rerank", lambda: fix.search_batch_reranked_device(store, nq, sp, k, qs.rows_dev, qs.ld, o["ids"], o["d"], o["ln"],
                                                                          o["st"], stream=o["s"]), sp.number_of_candidates)]
    for name, fn, stride in exact:
        t = [timed(fn, 1, 1 if i == 0 else 0) for i in range(args.runs)]
        out({"call": name, "ms": float(np.median(t)), "rounds": t, "spread_ms": round(max(t) - min(t), 4), "recall_at_10": recall(fn, stride)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--parent", default="", help="csrc directory of the parent commit, for the unchanged-kernels diff")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--candidates", default="64,256,1024")
    ap.add_argument("--tiles", default="0", help="forced row tiles (rows) the scan alone is timed under as well")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-index", action="store_true")
    args = ap.parse_args()
    resources(args) if args.resources else measure(args)


if __name__ == "__main__":
    main()
