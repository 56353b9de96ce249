"""The exhaustive MXFP4 scan (phnsw_fp4_scan_topk / _search, scan_fp4.hip) beside what the tree already had, on the
bench.py workload: the 1M x 768 clustered "survey" set, the same seeds and build, 10 000-query batches, k = 10, one
stream.  Writes profiles/fp4_scan/fp4_scan_profile.jsonl (the README there is written from it).  Nothing here is
asserted anywhere: the script reports what it finds, "slower than the walk" included.

  python scripts/fp4_scan_profile.py [--candidates 64,256,1024] [--steps 3 --warmup 1 --runs 3] [--no-index]
      the measurement (needs an MI355X).  Per r: ms per batch of the fp4 scan alone and of scan + f32 re-rank, and in the
      same process, ALTERNATING inside every round (machines differ by 10 %: a drift lands on all of them): the bits scan
      + re-rank, the fp4 graph walk + re-rank with r candidates, the f32 search at ef 256 / probe_depth 8, and once per
      run phnsw_search_exact_shared on the fp4 store with an all-ones bitmap (the exact path on the f32 MFMA tables).
      recall@10 against phnsw_bruteforce_topk on the f32 store.  Median and spread (max - min) of the rounds, and the
      block-scaled MFMA rate of the scan alone as a share of --peak (PFLOP/s, dense MXFP4 as AMD documents it).
      --no-index leaves out everything that needs the graph (its build takes most of the run).
  python scripts/fp4_scan_profile.py --resources [--parent DIR]
      needs only hipcc: the compiler's resource report of scan_fp4.hip (resource_usage_fp4_scan.txt) and, with --parent
      pointing at the csrc directory of the parent commit, resource_usage_existing_diff.txt: every kernel that exists in
      both trees and how many differ in a reported figure."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
CSRC = os.path.join(ROOT, "parallel_hnsw_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "fp4_scan")


def resources(args):
    import bits_profile as bp
    from concurrent.futures import ThreadPoolExecutor

    os.makedirs(OUT, exist_ok=True)
    bp.FLAGS[:0] = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
    mine = bp.resource_report(CSRC, "scan_fp4.hip")
    del bp.FLAGS[:4]
    with open(os.path.join(OUT, "resource_usage_fp4_scan.txt"), "w") as f:
        f.write("kernel | VGPRs | AGPRs | SGPRs | scratch bytes/lane | waves/SIMD | static LDS\n")
        for k in sorted(mine):
            r = mine[k]
            f.write("%s | %s | %s | %s | %s | %s | %s\n" % (k, r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"),
                                                        r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]"),
                                                        r.get("LDS Size [bytes/block]")))
        f.write("total: %d kernels\n" % len(mine))
    if not args.parent:
        return
    units = sorted(u for u in os.listdir(args.parent) if u.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        new = list(ex.map(lambda u: bp.resource_report(CSRC, u), units))
        old = list(ex.map(lambda u: bp.resource_report(args.parent, u), units))
    total = 0
    with open(os.path.join(OUT, "resource_usage_existing_diff.txt"), "w") as f:
        for u, a, b in zip(units, new, old):
            both = sorted(set(a) & set(b))
            differ = [k for k in both if a[k] != b[k]]
            total += len(both)
            f.write("%s: %d kernels of the parent commit, %d missing now, %d differ in a reported figure, %d new\n"
                    % (u, len(b), len(set(b) - set(a)), len(differ), len(set(a) - set(b))))
            for k in differ:
                f.write("  %s: %s -> %s\n" % (k, b[k], a[k]))
        f.write("total: %d kernels compared\n" % total)


def measure(args):
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, k = args.n, args.dim, args.nq, 10
    noise = 0.1 * dim ** 0.5
    make = lambda count, first: ph.VectorStore.clustered(count, dim, seed=42, first=first, n_clusters=1000, noise=noise)
    store, qs = make(n, 0), make(nq, 2 ** 32)
    gt = torch.empty((nq, k), dtype=torch.int32, device=dev)
    gd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    store.bruteforce_topk_device(qs.rows_dev, qs.ld, nq, k, gt.data_ptr(), gd.data_ptr())
    torch.cuda.synchronize()
    gt = gt.cpu().numpy()
    fp4, bits = ph.FP4Store.from_full(store), ph.BitStore.from_full(store)
    stream = torch.cuda.Stream()
    ids = torch.empty((nq, 1024), dtype=torch.int32, device=dev)
    d = torch.empty((nq, 1024), dtype=torch.float32, device=dev)
    ln = torch.empty(nq, dtype=torch.int32, device=dev)
    status = torch.zeros(nq, dtype=torch.int32, device=dev)
    out = dict(ids=ids.data_ptr(), d=d.data_ptr(), ln=ln.data_ptr(), st=status.data_ptr(), s=stream.cuda_stream)
    index = fix = None
    if not args.no_index:
        index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
        fix = ph.Hnsw.from_layers(fp4, [(l.nodes, l.neighbors) for l in index.layers], index.build_parameters)
        ones = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
    f32_sp = ph.SearchParameters(256, 256, 8)

    def timed(launch, steps=None, warmup=None):
        for _ in range(args.warmup if warmup is None else warmup):
            launch()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(steps or args.steps):
            launch()
        b.record(stream)
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any(), "a query failed"
        return round(a.elapsed_time(b) / (steps or args.steps), 4)

    def recall(stride):
        got = ids.cpu().numpy().reshape(-1)[: nq * stride].reshape(nq, stride)[:, :k]
        return float(np.mean([len(set(got[i].tolist()) & set(gt[i].tolist())) / float(k) for i in range(nq)]))

    lines = []
    for r in [int(x) for x in args.candidates.split(",")]:
        sp = ph.SearchParameters(r, r, args.probe_depth)
        calls = [("fp4_scan", lambda: fp4.scan_device(nq, r, qs.rows_dev, qs.ld, out["ids"], out["d"], out["ln"], stream=out["s"]), r),
                 ("fp4_scan_search", lambda: fp4.scan_search_device(store, nq, r, k, qs.rows_dev, qs.ld, out["ids"], out["d"], out["ln"],
                                                                    stream=out["s"]), r),
                 ("bits_scan_search", lambda: bits.scan_search_device(store, nq, r, k, qs.rows_dev, qs.ld, out["ids"], out["d"], out["ln"],
                                                                      stream=out["s"]), r)]
        if index is not None:
            calls.append(("f32_ef256", lambda: index.search_batch_device(nq, f32_sp, out["ids"], out["d"], out["ln"], out["st"],
                                                                         queries=qs.rows_dev, ldq=qs.ld, stream=out["s"]), 256))
            if r >= 256:
                calls.append(("fp4_walk_reranked", lambda: fix.search_batch_reranked_device(
                    store, nq, sp, k, qs.rows_dev, qs.ld, out["ids"], out["d"], out["ln"], out["st"], stream=out["s"]), r))
        runs = {name: [] for name, _, _ in calls}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
            for name, fn, _ in calls:
                runs[name].append(timed(fn))
        rec = {}
        for name, fn, stride in calls:
            fn()
            stream.synchronize()
            rec[name] = round(recall(stride), 4)
        ms = {v: float(np.median(runs[v])) for v in runs}
        steps128 = (dim + 127) // 128
        flops = 2.0 * 128 * steps128 * ((n + 15) // 16 * 16) * ((nq + 15) // 16 * 16)  # what the instructions execute
        line = {"r": r, "vectors": n, "dim": dim, "queries": nq, "rounds": runs, "ms": ms, "recall_at_10": rec,
                "spread_ms": {v: round(max(runs[v]) - min(runs[v]), 4) for v in runs},
                "fp4_scan_mfma_pflops": round(flops / (ms["fp4_scan"] * 1e-3) / 1e15, 4),
                "share_of_peak": round(flops / (ms["fp4_scan"] * 1e-3) / 1e15 / args.peak, 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if index is not None:  # the exact path the tree had: every row allowed, on the f32 MFMA tables over the widened operand
        shared = lambda: fix.search_exact_shared_device(nq, k, out["ids"], out["d"], out["ln"], out["st"], queries=qs.rows_dev,
                                                        ldq=qs.ld, allow=ones.data_ptr(), stream=out["s"])
        t = [timed(shared, steps=1, warmup=1) for _ in range(args.runs)]
        line = {"exact_shared_fp4_all_ones_ms": float(np.median(t)), "rounds": t, "spread_ms": round(max(t) - min(t), 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "fp4_scan_profile.jsonl"), "a") as f:
        f.write("\n".join(json.dumps(x) for x in lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--parent", default="", help="csrc directory of the parent commit, for the unchanged-kernels diff")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--candidates", default="64,256,1024")
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-index", action="store_true")
    ap.add_argument("--peak", type=float, default=10.1, help="dense MXFP4 peak of the device, PFLOP/s")
    args = ap.parse_args()
    resources(args) if args.resources else measure(args)


if __name__ == "__main__":
    main()
