"""The bits row store (1 sign bit per component, Hamming walk, f32 re-rank) beside the f32 search on the bench.py
workload: the 1M x 768 clustered "survey" set, the same seeds and build, 10 000-query batches, k = 10, one stream.
Writes the data files of profiles/bits/ (the README there is written from them).  Nothing here is asserted anywhere:
the script reports what it finds, "slower at equal recall" included.

  python scripts/bits_profile.py [--candidates 256,512,1024] [--steps 5 --warmup 2 --runs 3]
      the measurement (needs an MI355X).  Per setting of number_of_candidates for the bits store: ms per batch of the
      walk alone (phnsw_search_batch_device), of walk + re-rank (phnsw_bits_search_batch_device; the re-rank is the
      difference) and recall@10 of the re-ranked rows against phnsw_bruteforce_topk on the f32 store.  The f32 search at
      ef 256 / probe_depth 8 is timed IN THE SAME PROCESS, ALTERNATING with the bits calls inside every round, because
      machines differ by 10 %: a drift lands on both.  Median and spread (max - min) of the rounds.
  python scripts/bits_profile.py --resources [--parent DIR]
      needs only hipcc: the compiler's resource report of the 12 bits kernels (resource_usage_bits.txt) and, with
      --parent pointing at the csrc directory of the parent commit, resource_usage_existing_diff.txt: every kernel that
      exists in both trees, translation unit by translation unit, and how many differ in a reported figure."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "parallel_hnsw_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "bits")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
FIGURES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]",
           "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def resource_report(csrc, unit):
    """{kernel: {figure: value}} of one translation unit, from the compiler's remarks"""
    extra = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"] if unit == "tiny.hip" else []
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    err = subprocess.run([hipcc] + FLAGS + extra + [unit], cwd=csrc, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z\[\]/ ]+): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1).strip() in FIGURES:
            cur[m.group(1).strip()] = m.group(2)
    return out


def resources(args):
    os.makedirs(OUT, exist_ok=True)
    mine = resource_report(CSRC, "search_bits.hip")
    with open(os.path.join(OUT, "resource_usage_bits.txt"), "w") as f:
        f.write("kernel | VGPRs | SGPRs | scratch bytes/lane | waves/SIMD | static LDS\n")
        for k in sorted(mine):
            r = mine[k]
            f.write("%s | %s | %s | %s | %s | %s\n" % (k, r.get("VGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize [bytes/lane]"),
                                                   r.get("Occupancy [waves/SIMD]"), r.get("LDS Size [bytes/block]")))
        f.write("total: %d kernels\n" % len(mine))
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
            gone = sorted(set(b) - set(a))
            total += len(both)
            f.write("%s: %d kernels of the parent commit, %d missing now, %d differ in a reported figure, %d new\n"
                    % (u, len(b), len(gone), len(differ), len(set(a) - set(b))))
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
    store = make(n, 0)
    index = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters())
    qs = make(nq, 2 ** 32)
    gt = torch.empty((nq, k), dtype=torch.int32, device=dev)
    gd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    store.bruteforce_topk_device(qs.rows_dev, qs.ld, nq, k, gt.data_ptr(), gd.data_ptr())
    torch.cuda.synchronize()
    gt = gt.cpu().numpy()
    bits = ph.BitStore.from_full(store)
    bix = ph.Hnsw.from_layers(bits, [(l.nodes, l.neighbors) for l in index.layers], index.build_parameters)
    stream = torch.cuda.Stream()
    cap = 1024
    ids = torch.empty((nq, cap), dtype=torch.int32, device=dev)
    d = torch.empty((nq, cap), dtype=torch.float32, device=dev)
    ln = torch.empty(nq, dtype=torch.int32, device=dev)
    status = torch.empty(nq, dtype=torch.int32, device=dev)
    f32_sp = ph.SearchParameters(256, 256, 8)

    def f32():
        index.search_batch_device(nq, f32_sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qs.rows_dev,
                                  ldq=qs.ld, stream=stream.cuda_stream)

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

    def recall(stride):
        got = ids.cpu().numpy().reshape(-1)[: nq * stride].reshape(nq, stride)[:, :k]
        return float(np.mean([len(set(got[i].tolist()) & set(gt[i].tolist())) / float(k) for i in range(nq)]))

    lines = []
    for ef in [int(x) for x in args.candidates.split(",")]:
        sp = ph.SearchParameters(ef, ef, args.probe_depth)

        def walk():
            bix.search_batch_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qs.rows_dev,
                                    ldq=qs.ld, stream=stream.cuda_stream)

        def reranked():
            bix.search_batch_reranked_device(store, nq, sp, k, qs.rows_dev, qs.ld, ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                                             status.data_ptr(), stream=stream.cuda_stream)

        runs = {"f32": [], "walk": [], "reranked": []}
        for _ in range(args.runs):  # alternating: a drift of the machine lands on all three
            for name, fn in (("f32", f32), ("walk", walk), ("reranked", reranked)):
                runs[name].append(timed(fn))
        f32()
        torch.cuda.synchronize()
        r_f32 = recall(256)
        reranked()
        torch.cuda.synchronize()
        r_bits = recall(ef)
        med = {v: float(np.median(runs[v])) for v in runs}
        line = {"number_of_candidates": ef, "probe_depth": args.probe_depth, "vectors": n, "dim": dim, "queries": nq,
                "rounds": runs, "f32_ef256_ms": med["f32"], "bits_walk_ms": med["walk"], "bits_reranked_ms": med["reranked"],
                "rerank_ms": round(med["reranked"] - med["walk"], 4), "recall_at_10_bits_reranked": round(r_bits, 4),
                "recall_at_10_f32_ef256": round(r_f32, 4),
                "spread_ms": {v: round(max(runs[v]) - min(runs[v]), 4) for v in runs}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "bits_profile.jsonl"), "a") as f:
        f.write("\n".join(json.dumps(x) for x in lines) + "\n")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--parent", default="", help="csrc directory of the parent commit, for the unchanged-kernels diff")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--candidates", default="256,512,1024")
    ap.add_argument("--probe-depth", type=int, default=8)
    ap.add_argument("--vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", dest="nq", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if args.resources:
        resources(args)
    else:
        for x in measure(args):
            print("%d candidates: bits walk %.2f ms, + re-rank %.2f ms, recall@10 %.4f; f32 at ef 256: %.2f ms, recall@10 %.4f"
                  % (x["number_of_candidates"], x["bits_walk_ms"], x["bits_reranked_ms"], x["recall_at_10_bits_reranked"],
                     x["f32_ef256_ms"], x["recall_at_10_f32_ef256"]))


if __name__ == "__main__":
    main()
