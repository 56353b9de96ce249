#!/usr/bin/env python3
"""Resource usage of the PH_FM_LABEL_RANGE instances of the search kernels beside their PH_FM_RANGE siblings, from the
compiler's own report.

usage: resource_twins.py TREE OUT_DIR [HIPCC]

Cross-compiles (no GPU needed) search_ranged.hip and search_label_ranged.hip of TREE with
-Rpass-analysis=kernel-resource-usage, one log per unit under OUT_DIR, and prints every label-range instance (filter mode 32,
the last integer template argument) beside the range instance (mode 16) of the same shape, matched on the mangled name,
then how many label-range instances use more scratch or hold fewer waves per SIMD than their sibling.
"""
import concurrent.futures
import os
import re
import subprocess
import sys

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"]
FIG = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass")
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size", "VGPRs Spill", "SGPRs Spill")


def compile_unit(hipcc, tree, unit, log):
    src = os.path.join(tree, "parallel_hnsw_amd", "csrc", unit + ".hip")
    r = subprocess.run([hipcc] + FLAGS + [src, "-o", os.devnull], capture_output=True, text=True)
    open(log, "w").write(r.stderr)
    if r.returncode:
        raise SystemExit("%s failed to compile: see %s" % (src, log))
    return log


def parse(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = FIG.search(line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, [re.sub(r"\(.*", "", x).replace("void ", "") for x in r.stdout.split("\n")]))
    except Exception:
        return {n: n for n in names}


def main():
    tree, out = sys.argv[1], sys.argv[2]
    hipcc = sys.argv[3] if len(sys.argv) > 3 else "/opt/rocm/bin/hipcc"
    os.makedirs(out, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=2) as pool:
        jobs = {u: pool.submit(compile_unit, hipcc, tree, u, os.path.join(out, u + ".txt")) for u in ("search_ranged", "search_label_ranged")}
    lab, rng = parse(jobs["search_ranged"].result()), parse(jobs["search_label_ranged"].result())
    pretty = demangle(list(rng))
    print("| PH_FM_LABEL_RANGE instance | " + " | ".join("%s range | %s label-range" % (k, k) for k in KEYS) + " |")
    print("|---|" + "---|" * (2 * len(KEYS)))
    worse = unmatched = 0
    for n in sorted(rng, key=lambda x: pretty[x]):
        twin = lab.get(re.sub(r"Li32E(?=E+v12PhSearchArgs$)", "Li16E", n))
        if twin is None:
            unmatched += 1
            twin = {}
        cols = []
        for k in KEYS:
            cols += [twin.get(k, "-"), rng[n].get(k, "-")]
        bad = twin and ((int(rng[n].get("ScratchSize", 0)) > 0 and int(twin.get("ScratchSize", 0)) == 0) or
                        int(rng[n].get("Occupancy", 0)) < int(twin.get("Occupancy", 0)))
        worse += 1 if bad else 0
        print("| %s%s | %s |" % (pretty[n], " **" if bad else "", " | ".join(cols)))
    print("\n%d label-range instances (%d without a range sibling of that name); %d use scratch where the range sibling uses none or hold "
          "fewer waves per SIMD than it (marked **)" % (len(rng), unmatched, worse))


if __name__ == "__main__":
    main()
