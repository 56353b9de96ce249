#!/usr/bin/env python3
"""Compare two -Rpass-analysis=kernel-resource-usage logs of one unit by kernel name.

usage: resource_diff.py PARENT.txt CHANGED.txt UNIT
Prints "UNIT: N kernels, D differ in a reported figure", every differing figure, and a table of the kernels that
only CHANGED has, each beside its existing twin: the <..., true> (PAIRS) instance of the scan and tile kernels beside
the <...> instance, ph_labelset_X beside ph_labeled_X.  The scan and tile kernels gained a defaulted bool template
argument, which only shows in the mangled name (Lb0E): it is dropped before names are compared.
"""
import re
import subprocess
import sys

FIG = re.compile(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass")


def parse(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1).replace("Lb0EEv13PhLabeledArgs", "Ev13PhLabeledArgs")
            out[name] = {}
            continue
        m = FIG.search(line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except Exception:
        return {n: n for n in names}


def main():
    old, new, unit = parse(sys.argv[1]), parse(sys.argv[2]), sys.argv[3]
    differ = 0
    for name, figs in old.items():
        if name not in new:
            print("%s: MISSING in the changed build" % name)
            differ += 1
        elif new[name] != figs:
            differ += 1
            for k, v in figs.items():
                if new[name].get(k) != v:
                    print("%s: %s %s -> %s" % (name, k, v, new[name].get(k)))
    print("%s: %d kernels, %d differ in a reported figure" % (unit, len(old), differ))
    added = [n for n in new if n not in old]
    names = demangle(added + list(old))
    by_pretty = {re.sub(r"\(.*", "", names[n]).replace("void ", "").replace("> >", ">>"): old[n] for n in old}
    print("\n| new instance | VGPRs twin | VGPRs | SGPRs twin | SGPRs | scratch twin | scratch | waves/SIMD twin | waves/SIMD | "
          "VGPR spill twin | VGPR spill |\n|---|---|---|---|---|---|---|---|---|---|---|")
    for n in added:
        pretty = re.sub(r"\(.*", "", names[n]).replace("void ", "")
        twin = by_pretty.get(pretty.replace("ph_labelset_", "ph_labeled_").replace(", true>", ">"), {})
        f = new[n]
        cols = []
        for key in ("VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "VGPRs Spill"):
            cols += [twin.get(key, "-"), f.get(key, "-")]
        print("| %s | %s |" % (pretty, " | ".join(cols)))


if __name__ == "__main__":
    main()
