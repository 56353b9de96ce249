"""The filtered search (phnsw_search_batch_filtered_device) on the plain bench.py workload: the 1M x 768 clustered
"survey" set, the same seeds and build, ef 256 / probe_depth 8, 10 000-query batches on one stream.  Modes:

  unfiltered        phnsw_search_batch_device, as bench.py times it
  shared_1.0 / shared_0.5 / shared_0.1    one allow bitmap of that density for the whole batch
  per_query_0.5     one bitmap per query

Every mode reports ms per step from device events after warm-up (--runs repetitions, the spread beside the median),
queries per second, and the mean number of results per query (a post-filter: expect about ef x density).  One JSON line
per mode.

  python scripts/bench_filter.py [--modes unfiltered,shared_1.0,shared_0.5,shared_0.1,per_query_0.5] [--out FILE]

Mode `unfiltered` uses only calls that exist without the filtered search, so this file copied onto the parent checkout
gives the baseline: run it there and here alternately, three runs each, and judge this checkout's unfiltered rate against
the spread of the parent's runs (profiles/filter/README.md)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="unfiltered,shared_1.0,shared_0.5,shared_0.1,per_query_0.5")
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--ef", type=int, default=256)
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3, help="repetitions of every timed measurement (the spread is reported)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import parallel_hnsw_amd as ph

    dev = torch.device("cuda:0")
    n, dim, nq, ef = args.n, args.dim, args.nq, args.ef
    noise = 0.1 * dim ** 0.5
    store = ph.VectorStore.clustered(n, dim, seed=42, first=0, n_clusters=1000, noise=noise)
    index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
    qs = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 32, n_clusters=1000, noise=noise)
    sp = ph.SearchParameters(ef, ef, args.probe_depth)
    stream = torch.cuda.Stream()
    ids = torch.empty((nq, ef), dtype=torch.int32, device=dev)
    d = torch.empty((nq, ef), dtype=torch.float32, device=dev)
    ln = torch.empty(nq, dtype=torch.int32, device=dev)
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    nw = (n + 31) // 32
    out_lines = []
    for mode in args.modes.split(","):
        words, stride, density = None, 0, None
        if mode != "unfiltered":
            density = float(mode.rsplit("_", 1)[1])
            rows = nq if mode.startswith("per_query") else 1
            # bits drawn on the device: a [rows, n] bool mask packed into u32 words, 32 ids per word
            gen = torch.Generator(device=dev).manual_seed(7)
            words = torch.zeros((rows, nw), dtype=torch.int32, device=dev)
            for b in range(32):
                bit = (torch.rand((rows, nw), generator=gen, device=dev) < density).to(torch.int32)
                words |= bit << b if b < 31 else bit * -(2 ** 31)
            stride = nw if rows > 1 else 0

        def launch():
            if words is None:
                index.search_batch_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                          queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream)
            else:
                index.search_batch_filtered_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                                   queries=qs.rows_dev, ldq=qs.ld, allow=words.data_ptr(), allow_stride=stride,
                                                   stream=stream.cuda_stream)

        def timed():
            for _ in range(args.warmup):
                launch()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.steps):
                launch()
            b.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / args.steps

        runs = [round(timed(), 4) for _ in range(args.runs)]
        assert not status.cpu().numpy().any(), "a query failed"
        med = float(np.median(runs))
        line = {"mode": mode, "density": density, "vectors": n, "dim": dim, "queries": nq, "ef": ef,
                "probe_depth": args.probe_depth, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": {"runs": runs, "median": med, "spread": round(max(runs) - min(runs), 4)},
                "queries_per_second": round(nq / med * 1000.0, 1),
                "results_per_query": round(float(ln.cpu().numpy().astype(np.int64).mean()), 2),
                "expected_results_per_query": None if density is None else round(ef * density, 1)}
        print(json.dumps(line), flush=True)
        out_lines.append(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
