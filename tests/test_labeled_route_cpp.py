"""The pure functions the calls by label added to parallel_hnsw_amd/csrc/label_plan.h (the subset seeding of a lookup
position) and filter_route.h (the labeled scan_below default, the candidate test of exclude[q] on the label column) in a
stand-alone host program under AddressSanitizer and UBSan: tests/cpp/test_labeled_route.cpp, compiled with g++ and run
as a process of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_labeled_route_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_labeled_route")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_labeled_route.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
