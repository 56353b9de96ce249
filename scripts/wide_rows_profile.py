"""f32 rows of 1537 .. 4096 floats (DistF32Wide, search_wide.hip): the data files of profiles/wide_rows/ (the README
there is written from them).  Nothing here is asserted anywhere.

  python scripts/wide_rows_profile.py --resources [--parent DIR]
      needs only hipcc.  resource_usage_wide.txt: the compiler's report of the 12 kernels of search_wide.hip and of the
      wide instances of misc.hip and build.hip, as built.  resource_usage_shapes.txt: search_wide.hip compiled once per
      (P, U) of SHAPES -- chunks per piece, rows in flight -- the figures the choice in wide_rows.h was made from.  With
      --parent pointing at the csrc directory of the parent commit, resource_usage_existing_diff.txt: every kernel that
      exists in both trees, translation unit by translation unit, and how many differ in a reported figure.
  python scripts/wide_rows_profile.py [--vectors 200000 --dim 3072 --queries 10000 --ef 256 --steps 5 --warmup 2 --runs 3]
      the measurement (needs an MI355X): a synthetic f32 set, the index built on the device, batches of raw queries
      through phnsw_search_batch_device on one stream; ms per batch (host clock around a device synchronise), queries
      per second and evaluated rows x row bytes per second (the kernels' own evaluation counters).  Median and spread
      (max - min) of the runs; appends one line to wide_rows_profile.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bits_profile import CSRC, resource_report  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "wide_rows")
SHAPES = [(2, 4), (4, 4), (2, 8), (4, 8)]
HEAD = "kernel | VGPRs | AGPRs | SGPRs | scratch bytes/lane | VGPRs spilled | SGPRs spilled | waves/SIMD | static LDS\n"


def line(k, r):
    return "%s | %s | %s | %s | %s | %s | %s | %s | %s\n" % (
        k, r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill"),
        r.get("SGPRs Spill"), r.get("Occupancy [waves/SIMD]"), r.get("LDS Size [bytes/block]"))


def resources(args):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "resource_usage_wide.txt"), "w") as f:
        f.write(HEAD)
        total = 0
        for unit in ("search_wide.hip", "misc.hip", "build.hip"):
            rep = resource_report(CSRC, unit)
            for k in sorted(k for k in rep if "DistF32Wide" in k):
                f.write(line(k, rep[k]))
                total += 1
        f.write("total: %d kernels\n" % total)
    with open(os.path.join(OUT, "resource_usage_shapes.txt"), "w") as f:
        for p, u in SHAPES:
            rep = resource_report(CSRC, "search_wide.hip", ("PH_WIDE_P=%d" % p, "PH_WIDE_U=%d" % u))
            f.write("P = %d chunks per piece, U = %d rows in flight\n" % (p, u) + HEAD)
            for k in sorted(rep):
                f.write(line(k, rep[k]))
    if not args.parent:
        return
    from concurrent.futures import ThreadPoolExecutor
    units = sorted(u for u in os.listdir(args.parent) if u.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        new = list(ex.map(lambda u: resource_report(CSRC, u), units))
        old = list(ex.map(lambda u: resource_report(args.parent, u), units))
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
    store = ph.VectorStore.synthetic(args.n, args.dim, seed=42)
    t0 = time.time()
    index = ph.Hnsw.generate(store, np.arange(args.n), ph.BuildParameters(seed=1))
    build_s = time.time() - t0
    sp = ph.SearchParameters(args.ef, args.ef, 2)
    nq, ld = args.nq, (args.dim + 3) // 4 * 4
    qs = ph.VectorStore.synthetic(nq, args.dim, seed=42, first=2 ** 32)
    q = torch.from_numpy(np.ascontiguousarray(np.pad(qs.read(), ((0, 0), (0, ld - args.dim))))).cuda()
    ids = torch.empty((nq, args.ef), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, args.ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    stats = torch.zeros((nq, 2), dtype=torch.int32, device="cuda")

    def batch():
        index.search_batch_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=q.data_ptr(),
                                  ldq=ld, out_stats=stats.data_ptr())

    ms = []
    for _ in range(args.runs):
        for _ in range(args.warmup):
            batch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            batch()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    assert int(status.abs().sum()) == 0
    evals = int(stats[:, 0].to(torch.int64).sum())  # rows evaluated by one batch
    med = float(np.median(ms))
    rec = {"vectors": args.n, "dim": args.dim, "queries": nq, "ef": args.ef, "layers": [len(index._layer(l).nodes) for l in range(index.layer_count())],
           "build_s": round(build_s, 1), "ms_per_batch": [round(m, 3) for m in ms], "ms_median": round(med, 3),
           "ms_spread": round(max(ms) - min(ms), 3), "queries_per_s": round(nq / med * 1e3), "rows_evaluated_per_batch": evals,
           "row_bytes": ld * 4, "gathered_GB_per_s": round(evals * ld * 4 / med / 1e6, 1)}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "wide_rows_profile.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--parent", default="", help="csrc directory of the parent commit, for the unchanged-kernels diff")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--vectors", dest="n", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=3072)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--ef", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    resources(args) if args.resources else measure(args)


if __name__ == "__main__":
    main()
