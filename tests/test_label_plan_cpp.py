"""The integer rules of the exact search by row label (parallel_hnsw_amd/csrc/label_plan.h: slice ranges over a list's
64-id batches, the tile size T and its LDS, label slots, scratch sizes) and a host model of the tile cut over sorted
slots, in a stand-alone host program under AddressSanitizer and UBSan: tests/cpp/test_label_plan.cpp, compiled with g++
and run as a process of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_label_plan_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_label_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_label_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
