"""The integer rules of the exact scan over an allow-list (parallel_hnsw_amd/csrc/exact_slices.h: k and stride checks,
slice count, pass ranges, LDS layout) in a stand-alone host program under AddressSanitizer and UBSan: tests/cpp/
test_exact_slices.cpp, compiled with g++ and run as a process of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_slice_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_exact_slices")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_exact_slices.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
