"""The pure functions the calls by a set of row labels added to parallel_hnsw_amd/csrc/filter_route.h (the soundness test of
the untrusted offsets, the membership predicate of the walk, the candidate test of exclude[q], the scan_below default of the
routed call) in a stand-alone host program under AddressSanitizer and UBSan: tests/cpp/test_labelset_route.cpp, compiled
with g++ and run as a process of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_labelset_route_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_labelset_route")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_labelset_route.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
