#!/usr/bin/env python3
"""Resource usage of the PH_FM_LABELSET_RANGE instances of the search kernels beside their PH_FM_LABELSET and
PH_FM_LABEL_RANGE siblings, from the compiler's own report.

usage: resource_twins.py TREE OUT_DIR [HIPCC] [--reuse]

Cross-compiles (no GPU needed) search_labelset.hip, search_label_ranged.hip and search_labelset_ranged.hip of TREE with
-Rpass-analysis=kernel-resource-usage, the last one twice: as shipped (the two bounds read once per query in front of
the walk) and with -DPH_LABELSET_RANGE_BOUNDS_AT_TEST (the bounds read where the test runs).  One log per compile under
OUT_DIR; --reuse keeps a log that is already there.  Prints every set-range instance (filter mode 64, the last integer
template argument) beside the set instance (mode 8) and the label-range instance (mode 32) of the same shape, matched on
the mangled name, for VGPRs, scratch and waves per SIMD, then how many instances of either form miss the target: scratch
where the set sibling has none, or fewer waves per SIMD than the set sibling.
"""
import concurrent.futures
import os
import re
import subprocess
import sys

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"]
FIG = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass")
KEYS = ("VGPRs", "ScratchSize", "Occupancy")
UNITS = (("search_labelset", "search_labelset", []), ("search_label_ranged", "search_label_ranged", []),
         ("search_labelset_ranged", "search_labelset_ranged", []),
         ("search_labelset_ranged_at_test", "search_labelset_ranged", ["-DPH_LABELSET_RANGE_BOUNDS_AT_TEST"]))


def compile_unit(hipcc, tree, unit, extra, log, reuse):
    if reuse and os.path.exists(log) and os.path.getsize(log):
        return log
    src = os.path.join(tree, "parallel_hnsw_amd", "csrc", unit + ".hip")
    r = subprocess.run([hipcc] + FLAGS + extra + [src, "-o", os.devnull], capture_output=True, text=True)
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


def misses(inst, twin):
    return bool(twin) and ((int(inst.get("ScratchSize", 0)) > 0 and int(twin.get("ScratchSize", 0)) == 0) or
                           int(inst.get("Occupancy", 0)) < int(twin.get("Occupancy", 0)))


def main():
    args = [a for a in sys.argv[1:] if a != "--reuse"]
    reuse = "--reuse" in sys.argv[1:]
    tree, out = args[0], args[1]
    hipcc = args[2] if len(args) > 2 else "/opt/rocm/bin/hipcc"
    os.makedirs(out, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        jobs = {name: pool.submit(compile_unit, hipcc, tree, unit, extra, os.path.join(out, name + ".txt"), reuse)
                for name, unit, extra in UNITS}
    res = {name: parse(job.result()) for name, job in jobs.items()}
    new, at_test = res["search_labelset_ranged"], res["search_labelset_ranged_at_test"]
    pretty = demangle(list(new))
    heads = []
    for k in KEYS:
        heads += ["%s set" % k, "%s label-range" % k, "%s set-range" % k, "%s set-range, bounds at the test" % k]
    print("| PH_FM_LABELSET_RANGE instance | " + " | ".join(heads) + " |")
    print("|---|" + "---|" * len(heads))
    bad = bad_pq = unmatched = 0
    for n in sorted(new, key=lambda x: pretty[x]):
        twin = lambda mode: re.sub(r"Li64E(?=E+v12PhSearchArgs$)", "Li%dE" % mode, n)
        st, lr, pq = res["search_labelset"].get(twin(8), {}), res["search_label_ranged"].get(twin(32), {}), at_test.get(n, {})
        unmatched += 0 if st and lr and pq else 1
        cols = []
        for k in KEYS:
            cols += [st.get(k, "-"), lr.get(k, "-"), new[n].get(k, "-"), pq.get(k, "-")]
        b, bq = misses(new[n], st), misses(pq, st)
        bad += b
        bad_pq += bq
        print("| %s%s%s | %s |" % (pretty[n], " **" if b else "", " ++" if bq else "", " | ".join(cols)))
    print("\n%d set-range instances (%d without a sibling of that name in every unit); as shipped %d use scratch where the set "
          "sibling uses none or hold fewer waves per SIMD than it (marked **); with the bounds read where the test runs %d do (marked ++)"
          % (len(new), unmatched, bad, bad_pq))


if __name__ == "__main__":
    main()
