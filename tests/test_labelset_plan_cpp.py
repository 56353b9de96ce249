"""The integer rules of the exact search by label sets (parallel_hnsw_amd/csrc/labelset_plan.h: which query owns a pair
when the offsets cannot be trusted, range validity, the grouping block with the owner, inverse and duplicate arrays, the
key scratch in 64 bits) and a host model of the call -- claim, sort by slot, adjacent-duplicate flags, inverse, gather
per query -- against a brute-force union, in a stand-alone host program under AddressSanitizer and UBSan:
tests/cpp/test_labelset_plan.cpp, compiled with g++ and run as a process of its own.  No GPU, nothing loaded into
Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_labelset_plan_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_labelset_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_labelset_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
