"""The integer rules of the search by a set of row labels and a numeric range (parallel_hnsw_amd/csrc/labelset_range_plan.h
on top of labelset_plan.h and label_range_plan.h: the span per pair, the duplicate rule on the span-start order, the
count; filter_route.h: ph_pairset_holds, the walk's test, and the candidate test of the routed call; claims over offsets
that overlap and run backwards) against brute force on random columns, in a stand-alone host program under
AddressSanitizer and UBSan: tests/cpp/test_labelset_range_plan.cpp, compiled with g++ and run as a process of its own.
No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_labelset_range_plan_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_labelset_range_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_labelset_range_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
