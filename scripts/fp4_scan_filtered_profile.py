"""The MXFP4 scan over an allow-list (phnsw_fp4_scan_search_filtered, scan_fp4_filtered.hip) beside the exact filtered
calls the tree already had, on the bench.py workload: the 1M x 768 clustered "survey" set, 10 000-query batches, k = 10,
one stream, device forms, device-event times.  Appends to profiles/fp4_scan_filtered/fp4_scan_filtered_profile.jsonl (the
README there is written from it).  Nothing here is asserted anywhere: the script reports what it finds.

  python scripts/fp4_scan_filtered_profile.py [--candidates 64,256] [--density 0.01,0.1,0.5,1.0] [--runs 3] [--no-index]
      the measurement (needs an MI355X).  Per r and per shared mask of the given density: ms per batch of the LIST form +
      re-rank, of the MASK form with that mask repeated per query + re-rank and of the unfiltered phnsw_fp4_scan_search,
      ALTERNATING inside every round; recall@10 against the f32 brute-force top-10 of the allowed rows (a large-k
      brute force is not there: the ground truth is phnsw_search_exact_shared on the f32 store, which is exact).
      Then, once per mask, phnsw_search_exact_shared and (--filtered-density, it is slow) phnsw_search_exact_filtered
      on the fp4 store.  Median and spread (max - min) of the rounds.  --no-index leaves out everything that needs the
      graph, the ground truth and the recall included.
  python scripts/fp4_scan_filtered_profile.py --resources [--parent DIR]
      needs only hipcc: the compiler's resource report of scan_fp4_filtered.hip (resource_usage_fp4_scan_filtered.txt)
      and, with --parent pointing at the csrc directory of the parent commit, resource_usage_existing_diff.txt."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "fp4_scan_filtered")


def resources(args):
    import bits_profile as bp
    import fp4_scan_profile as fp

    fp.OUT = OUT
    os.makedirs(OUT, exist_ok=True)
    fp.resources(args)  # the unfiltered unit's report and the diff against the parent, into OUT
    os.remove(os.path.join(OUT, "resource_usage_fp4_scan.txt"))  # profiles/fp4_scan/ has it
    bp.FLAGS[:0] = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
    mine = bp.resource_report(fp.CSRC, "scan_fp4_filtered.hip")
    del bp.FLAGS[:4]
    with open(os.path.join(OUT, "resource_usage_fp4_scan_filtered.txt"), "w") as f:
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
    fp4 = ph.FP4Store.from_full(store)
    stream = torch.cuda.Stream()
    ids = torch.empty((nq, 1024), dtype=torch.int32, device=dev)
    d = torch.empty((nq, 1024), dtype=torch.float32, device=dev)
    ln = torch.empty(nq, dtype=torch.int32, device=dev)
    status = torch.zeros(nq, dtype=torch.int32, device=dev)
    o = dict(ids=ids.data_ptr(), d=d.data_ptr(), ln=ln.data_ptr(), st=status.data_ptr(), s=stream.cuda_stream)
    index = fix = None
    if not args.no_index:
        index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
        fix = ph.Hnsw.from_layers(fp4, [(l.nodes, l.neighbors) for l in index.layers], index.build_parameters)
    nw = (n + 31) // 32

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

    def out(line):
        print(json.dumps(line), flush=True)
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "fp4_scan_filtered_profile.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")

    for density in [float(x) for x in args.density.split(",")]:
        allow = np.random.default_rng(17).random(n) < density if density < 1.0 else np.ones(n, dtype=np.bool_)
        words, _ = ph.hnsw.pack_allow(allow, n, nq)
        shared = torch.from_numpy(words.view(np.int32)).to(dev)
        per_query = shared.repeat(nq, 1).contiguous()  # the same mask for every query: [nq, nw]
        gt = None
        if index is not None:  # exact on the f32 store: the f32 top-10 of the allowed rows
            index.search_exact_shared_device(nq, k, o["ids"], o["d"], o["ln"], o["st"], queries=qs.rows_dev, ldq=qs.ld,
                                             allow=shared.data_ptr(), stream=o["s"])
            stream.synchronize()
            gt = top(k)
        for r in [int(x) for x in args.candidates.split(",")]:
            calls = [("list", lambda: fp4.scan_search_filtered_device(store, nq, r, k, qs.rows_dev, qs.ld, shared.data_ptr(), 0, o["ids"],
                                                                      o["d"], o["ln"], stream=o["s"])),
                     ("mask", lambda: fp4.scan_search_filtered_device(store, nq, r, k, qs.rows_dev, qs.ld, per_query.data_ptr(), nw,
                                                                      o["ids"], o["d"], o["ln"], stream=o["s"])),
                     ("unfiltered", lambda: fp4.scan_search_device(store, nq, r, k, qs.rows_dev, qs.ld, o["ids"], o["d"], o["ln"],
                                                                   stream=o["s"]))]
            runs = {name: [] for name, _ in calls}
            for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
                for name, fn in calls:
                    runs[name].append(timed(fn, args.steps, args.warmup))
            rec = {}
            for name, fn in calls[:2]:
                fn()
                stream.synchronize()
                got = top(r)
                if gt is not None:
                    rec[name] = round(float(np.mean([len(set(got[i].tolist()) & set(gt[i].tolist())) / float(k) for i in range(nq)])), 4)
            out({"density": density, "allowed": int(allow.sum()), "r": r, "vectors": n, "dim": dim, "queries": nq, "rounds": runs,
                 "ms": {v: float(np.median(runs[v])) for v in runs}, "spread_ms": {v: round(max(runs[v]) - min(runs[v]), 4) for v in runs},
                 "recall_at_10_of_allowed": rec})
        if fix is not None:
            exact = [("exact_shared_fp4", lambda: fix.search_exact_shared_device(nq, k, o["ids"], o["d"], o["ln"], o["st"], queries=qs.rows_dev,
                                                                                  ldq=qs.ld, allow=shared.data_ptr(), stream=o["s"]))]
            if density <= args.filtered_density:
                exact.append(("exact_filtered_fp4", lambda: fix.search_exact_filtered_device(
                    nq, k, o["ids"], o["d"], o["ln"], o["st"], queries=qs.rows_dev, ldq=qs.ld, allow=shared.data_ptr(), stream=o["s"])))
            for name, fn in exact:
                t = [timed(fn, 1, 1 if i == 0 else 0) for i in range(args.runs)]
                out({"density": density, "call": name, "ms": float(np.median(t)), "rounds": t, "spread_ms": round(max(t) - min(t), 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--parent", default="", help="csrc directory of the parent commit, for the unchanged-kernels diff")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--candidates", default="64,256")
    ap.add_argument("--density", default="0.01,0.1,0.5,1.0")
    ap.add_argument("--filtered-density", type=float, default=0.1, help="phnsw_search_exact_filtered up to this density only")
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
