"""The integer rules of the filtered int8 scan (parallel_hnsw_amd/csrc/i8q_scan_filter_plan.h: the list-position clamp of a
row tile wider than the list's padding, the tile count from m, the LDS with the id ring) in a stand-alone host program
under AddressSanitizer and UBSan: tests/cpp/test_i8q_scan_filter_plan.cpp, compiled with g++ and run as a process of its
own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_i8q_scan_filter_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_i8q_scan_filter_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_i8q_scan_filter_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
