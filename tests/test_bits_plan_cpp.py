"""The layout rules of the bits row store (parallel_hnsw_amd/csrc/bits_plan.h: the sign rule, words per row, stride,
position of component j, padding, the value a Hamming distance stands for) in a stand-alone host program under
AddressSanitizer and UBSan: tests/cpp/test_bits_plan.cpp, compiled with g++ and run as a process of its own, over every
dimension 1 .. 1536 with a host model of the conversion and of the distance's row indexing.  No GPU, nothing loaded
into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bits_layout_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_bits_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_bits_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
