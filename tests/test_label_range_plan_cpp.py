"""The integer rules of the search by a row label and a numeric range (parallel_hnsw_amd/csrc/label_range_plan.h: the
span of a (label, range) pair in a column sorted by (label << 32) | key against a brute-force count, the sort key of
empty spans; filter_route.h: ph_pair_holds, the walk's test, and the candidate test of the routed call) in a stand-alone
host program under AddressSanitizer and UBSan: tests/cpp/test_label_range_plan.cpp, compiled with g++ and run as a
process of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_label_range_plan_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_label_range_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_label_range_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
