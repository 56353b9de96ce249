"""The integer rules of the exact search over a table of allow-lists (parallel_hnsw_amd/csrc/group_plan.h: selector keys,
rounds under the list budget, scratch sizes) and host models of its grouping pass, of its candidate lists and of the
select's `order` indexing, in a stand-alone host program under AddressSanitizer and UBSan: tests/cpp/test_group_plan.cpp,
compiled with g++ and run as a process of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_plan_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_group_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_group_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
