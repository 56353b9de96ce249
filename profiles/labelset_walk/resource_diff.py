#!/usr/bin/env python3
"""Resource usage of the search kernel instances of two source trees, from the compiler's own report.

usage: resource_diff.py PARENT_TREE CHANGED_TREE OUT_DIR [HIPCC]

Cross-compiles (no GPU needed) every translation unit of search kernels of both trees with
-Rpass-analysis=kernel-resource-usage, one log per unit under OUT_DIR, then prints
  - per unit both trees have: how many kernels, and every figure that differs (none is the expectation);
  - the instances only CHANGED has (the PH_FM_LABELSET twins, filter mode 8) beside their PH_FM_LABEL twins (mode 2).
The filter mode is the last integer template argument of every kernel; the twins are matched on the mangled name.
"""
import concurrent.futures
import os
import re
import subprocess
import sys

UNITS = ["search", "search_filtered", "search_labeled", "search_collect", "search_collect_labeled", "search_labelset"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"]
FIG = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass")
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size", "VGPRs Spill", "SGPRs Spill")


def compile_unit(hipcc, tree, unit, log):
    src = os.path.join(tree, "parallel_hnsw_amd", "csrc", unit + ".hip")
    if not os.path.exists(src):
        return None
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
    parent, changed, out = sys.argv[1], sys.argv[2], sys.argv[3]
    hipcc = sys.argv[4] if len(sys.argv) > 4 else "/opt/rocm/bin/hipcc"
    os.makedirs(out, exist_ok=True)
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=6) as pool:
        for tag, tree in (("parent", parent), ("changed", changed)):
            for u in UNITS:
                jobs[(tag, u)] = pool.submit(compile_unit, hipcc, tree, u, os.path.join(out, "%s_%s.txt" % (tag, u)))
    logs = {k: f.result() for k, f in jobs.items()}
    total = differ = 0
    for u in UNITS:
        if not logs[("parent", u)]:
            continue
        old, new = parse(logs[("parent", u)]), parse(logs[("changed", u)])
        d = 0
        for name, figs in old.items():
            if name not in new:
                print("%s: %s: MISSING in the changed tree" % (u, name))
                d += 1
            elif new[name] != figs:
                d += 1
                for k, v in figs.items():
                    if new[name].get(k) != v:
                        print("%s: %s: %s %s -> %s" % (u, name, k, v, new[name].get(k)))
        extra = [n for n in new if n not in old]
        print("%s.hip: %d kernels, %d differ in a reported figure, %d only in the changed tree" % (u, len(old), d, len(extra)))
        total += len(old)
        differ += d
    print("existing instances: %d, differing: %d" % (total, differ))
    # the new unit beside the label unit: filter mode 8 against filter mode 2
    lab, st = parse(logs[("changed", "search_labeled")]), parse(logs[("changed", "search_labelset")])
    pretty = demangle(list(st))
    print("\n| PH_FM_LABELSET instance | " + " | ".join("%s label | %s set" % (k, k) for k in KEYS) + " |")
    print("|---|" + "---|" * (2 * len(KEYS)))
    worse = 0
    for n in sorted(st, key=lambda x: pretty[x]):
        twin = lab.get(re.sub(r"Li8E(?=E+v12PhSearchArgs$)", "Li2E", n), {})
        cols = []
        for k in KEYS:
            cols += [twin.get(k, "-"), st[n].get(k, "-")]
        if twin and (int(st[n].get("ScratchSize", 0)) > int(twin.get("ScratchSize", 0)) or
                     int(st[n].get("Occupancy", 0)) < int(twin.get("Occupancy", 0))):
            worse += 1
        print("| %s | %s |" % (pretty[n], " | ".join(cols)))
    print("\n%d set instances, %d with more scratch or fewer waves per SIMD than their label twin" % (len(st), worse))


if __name__ == "__main__":
    main()
