"""The int8 scan over an allow-list (phnsw_i8q_scan_topk_filtered / _search_filtered, scan_i8q_filtered.hip) beside the
unfiltered int8 scan, the fp4 LIST form and the exact filtered calls the tree already had, on the bench.py workload: the
1M x 768 clustered "survey" set, 10 000-query batches, k = 10, one stream, one process, device forms, device-event times.
Appends to profiles/i8q_scan_filtered/i8q_scan_filtered_profile.jsonl (the README there is written from it).  Nothing here
is asserted anywhere: the script reports what it finds.

  python scripts/i8q_scan_filtered_profile.py [--candidates 64,256] [--density 0.01,0.1,0.5,1.0] [--runs 3] [--no-index]
      the measurement (needs an MI355X).  Per r and per shared mask of the given density: ms per batch of the LIST form and
      of the MASK form (that mask repeated per query), each alone and + re-rank, of the unfiltered int8 scan alone and
      + re-rank and of the fp4 LIST form + re-rank, ALTERNATING inside every round; recall@10 of the scan alone and of
      scan + re-rank against the exact f32 top-10 of the allowed rows (phnsw_search_exact_shared on the f32 store).
      Then, once per mask, phnsw_search_exact_shared and (--filtered-density, it is slow) phnsw_search_exact_filtered on
      the i8q store.  Median and spread (max - min) of the rounds.  --no-index leaves out everything that needs the
      graph, the ground truth and the recall included.
  python scripts/i8q_scan_filtered_profile.py --resources [--parent DIR]
      needs only hipcc: the compiler's resource report of scan_i8q_filtered.hip (resource_usage_i8q_scan_filtered.txt)
      and, with --parent pointing at the csrc directory of the parent commit, resource_usage_existing_diff.txt."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "i8q_scan_filtered")


def resources(args):
    import bits_profile as bp
    import fp4_scan_profile as fp

    fp.OUT = OUT
    os.makedirs(OUT, exist_ok=True)
    fp.resources(args)  # the fp4 unit's report and the diff of every existing unit against the parent, into OUT
    os.remove(os.path.join(OUT, "resource_usage_fp4_scan.txt"))  # profiles/fp4_scan/ has it
    mine = bp.resource_report(fp.CSRC, "scan_i8q_filtered.hip")
    with open(os.path.join(OUT, "resource_usage_i8q_scan_filtered.txt"), "w") as f:
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
    index = fix = None
    if not args.no_index:
        index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
        fix = ph.Hnsw.from_layers(i8q, [(l.nodes, l.neighbors) for l in index.layers], index.build_parameters)
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
        with open(os.path.join(OUT, "i8q_scan_filtered_profile.jsonl"), "a") as f:
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
            q = (nq, r, qs.rows_dev, qs.ld)
            qk = (store, nq, r, k, qs.rows_dev, qs.ld)
            res = (o["ids"], o["d"], o["ln"])
            calls = [("list", lambda: i8q.scan_filtered_device(*q, shared.data_ptr(), 0, *res, stream=o["s"])),
                     ("list_rerank", lambda: i8q.scan_search_filtered_device(*qk, shared.data_ptr(), 0, *res, stream=o["s"])),
                     ("mask", lambda: i8q.scan_filtered_device(*q, per_query.data_ptr(), nw, *res, stream=o["s"])),
                     ("mask_rerank", lambda: i8q.scan_search_filtered_device(*qk, per_query.data_ptr(), nw, *res, stream=o["s"])),
                     ("unfiltered", lambda: i8q.scan_device(*q, *res, stream=o["s"])),
                     ("unfiltered_rerank", lambda: i8q.scan_search_device(*qk, *res, stream=o["s"])),
                     ("fp4_list_rerank", lambda: fp4.scan_search_filtered_device(*qk, shared.data_ptr(), 0, *res, stream=o["s"]))]
            runs = {name: [] for name, _ in calls}
            for _ in range(args.runs):  # alternating: a drift of the machine lands on all of them
                for name, fn in calls:
                    runs[name].append(timed(fn, args.steps, args.warmup))
            rec = {}
            for name, fn in calls[:4]:
                fn()
                stream.synchronize()
                got = top(r)
                if gt is not None:
                    rec[name] = round(float(np.mean([len(set(got[i].tolist()) & set(gt[i].tolist())) / float(k) for i in range(nq)])), 4)
            out({"density": density, "allowed": int(allow.sum()), "r": r, "vectors": n, "dim": dim, "queries": nq, "rounds": runs,
                 "ms": {v: float(np.median(runs[v])) for v in runs}, "spread_ms": {v: round(max(runs[v]) - min(runs[v]), 4) for v in runs},
                 "recall_at_10_of_allowed": rec})
        if fix is not None:
            exact = [("exact_shared_i8q", lambda: fix.search_exact_shared_device(nq, k, o["ids"], o["d"], o["ln"], o["st"], queries=qs.rows_dev,
                                                                                  ldq=qs.ld, allow=shared.data_ptr(), stream=o["s"]))]
            if density <= args.filtered_density:
                exact.append(("exact_filtered_i8q", lambda: fix.search_exact_filtered_device(
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
