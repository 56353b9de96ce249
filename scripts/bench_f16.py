"""f32 search against f16, i8 and i8q search (and each + f32 re-rank) on the plain bench.py workload: the 1M x 768
clustered "survey" set, the same seeds and build, ef 256 / probe_depth 8, 10 000-query batches, one stream and two
streams (two batches in flight).  Every mode reports ms per step from device events after warm-up, recall@10
against the exact top 10 of the f32 store, and the dispatches of its last descent.  One JSON line per mode.

  python scripts/bench_f16.py --modes f32,f16,f16_rerank,i8,i8_rerank,i8q,i8q_rerank [--steps 20 --warmup 3] [--out FILE]

Mode f32 uses only calls that exist without the f16 and i8 stores, so this file copied onto an older checkout gives the
baseline of the same run (pass --modes f32 there)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f32,f16,f16_rerank,i8,i8_rerank,i8q,i8q_rerank")
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
    from parallel_hnsw_amd._lib import check, lib
    from parallel_hnsw_amd.hnsw import _p

    dev = torch.device("cuda:0")
    n, dim, nq, ef = args.n, args.dim, args.nq, args.ef
    noise = 0.1 * dim ** 0.5

    def make(count, first):
        return ph.VectorStore.clustered(count, dim, seed=42, first=first, n_clusters=1000, noise=noise)

    store = make(n, 0)
    index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
    qstores = [make(nq, 2 ** 32), make(nq, 2 ** 35)]
    sp = ph.SearchParameters(ef, ef, args.probe_depth)
    gts = []
    for qs in qstores:
        gt = torch.empty((nq, 10), dtype=torch.int32, device=dev)
        gd = torch.empty((nq, 10), dtype=torch.float32, device=dev)
        store.bruteforce_topk_device(qs.rows_dev, qs.ld, nq, 10, gt.data_ptr(), gd.data_ptr())
        torch.cuda.synchronize()
        gts.append(gt.cpu().numpy())
    s0 = torch.cuda.Stream()
    s1 = torch.cuda.ExternalStream(ph.stream_create_beside(0, s0.cuda_stream), device=dev)
    streams = [s0, s1]

    class Lane:
        def __init__(self):
            self.ids = torch.empty((nq, ef), dtype=torch.int32, device=dev)
            self.d = torch.empty((nq, ef), dtype=torch.float32, device=dev)
            self.len = torch.empty(nq, dtype=torch.int32, device=dev)
            self.status = torch.empty(nq, dtype=torch.int32, device=dev)

    lanes = [Lane(), Lane()]
    converted = {}  # "f16" / "i8" / "i8q" -> the index over that store, made when the first mode asks for it
    row_bytes = {"f32": 4 * int(store.ld), "f16": 2 * int(store.ld), "i8": (4 + int(store.ld) + 15) // 16 * 16}
    row_bytes["i8q"] = row_bytes["i8"]
    out_lines = []
    for mode in args.modes.split(","):
        kind = mode.split("_")[0]
        if kind != "f32" and kind not in converted:
            low = {"f16": ph.F16Store, "i8": ph.I8Store, "i8q": ph.I8QStore}[kind].from_full(store)
            converted[kind] = ph.Hnsw.from_layers(low, [(l.nodes, l.neighbors) for l in index.layers], index.build_parameters)
        ix = index if kind == "f32" else converted[kind]

        def launch(b, stream):
            ln, qs = lanes[b], qstores[b]
            if mode.endswith("_rerank"):
                ix.search_batch_reranked_device(store, nq, sp, 10, qs.rows_dev, qs.ld, ln.ids.data_ptr(), ln.d.data_ptr(),
                                                ln.len.data_ptr(), ln.status.data_ptr(), stream=stream.cuda_stream)
            else:
                ix.search_batch_device(nq, sp, ln.ids.data_ptr(), ln.d.data_ptr(), ln.len.data_ptr(), ln.status.data_ptr(),
                                       queries=qs.rows_dev, ldq=qs.ld, stream=stream.cuda_stream)

        def timed(two):
            """ms per step over K steps after W warm-up steps, from device events on the streams used"""
            pick = (lambda i: i & 1) if two else (lambda i: 0)
            for i in range(args.warmup):
                launch(pick(i), streams[pick(i)])
            torch.cuda.synchronize()
            used = streams if two else streams[:1]
            start = [torch.cuda.Event(enable_timing=True) for _ in used]
            end = [torch.cuda.Event(enable_timing=True) for _ in used]
            for s, e in zip(used, start):
                e.record(s)
            for i in range(args.steps):
                launch(pick(i), streams[pick(i)])
            for s, e in zip(used, end):
                e.record(s)
            torch.cuda.synchronize()
            # the streams start together (after the synchronize): the step time is the longest stream's span over K
            return max(a.elapsed_time(b) for a, b in zip(start, end)) / args.steps

        one = [round(timed(False), 4) for _ in range(args.runs)]
        two = [round(timed(True), 4) for _ in range(args.runs)]
        recalls = []
        for b in range(2):
            assert not lanes[b].status.cpu().numpy().any(), "a query failed"
            ids = lanes[b].ids.cpu().numpy()[:, :10]
            recalls.append(float(np.mean([len(set(ids[i].tolist()) & set(gts[b][i].tolist())) / 10.0 for i in range(nq)])))
        cap = 32
        cnt = C.c_uint32()
        ms = np.zeros(cap, dtype=np.float32)
        nd, nh = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
        lo, hi = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        check(lib().phnsw_last_search_dispatches(ix._h, cap, C.byref(cnt), _p(ms), _p(nd), _p(nh), _p(lo), _p(hi)))
        disp = [{"layers": "dense top layers" if i == 0 else "%d-%d" % (lo[i], hi[i] - 1), "ms": round(float(ms[i]), 3),
                 "distance_evals": int(nd[i])} for i in range(cnt.value)]
        line = {"mode": mode, "vectors": n, "dim": dim, "queries": nq, "ef": ef, "probe_depth": args.probe_depth,
                "steps": args.steps, "warmup": args.warmup,
                "one_stream_ms_per_step": {"runs": one, "median": float(np.median(one)), "spread": round(max(one) - min(one), 4)},
                "two_streams_ms_per_step": {"runs": two, "median": float(np.median(two)), "spread": round(max(two) - min(two), 4)},
                "recall_at_10": [round(r, 4) for r in recalls], "last_search_dispatches": disp,
                "store_bytes": int(n) * row_bytes[kind],
                "layers": [int(l.node_count()) for l in index.layers]}
        print(json.dumps(line), flush=True)
        out_lines.append(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
