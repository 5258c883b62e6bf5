"""The two-source row sums (csrc/rowsum.hpp) on the host: tests/native/rowsum2_test.cpp runs
rowsum2_word against a direct double loop at L = 3 and L = 2049 with A and B in separate allocations, what rowplan2_ok
refuses, and the plan of a GCM call over key tables (three frames, two slots, m = 1, 2, 4) on plain bits against the
single-key plans and GHASH -- plain and as a -fsanitize=address,undefined binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_rowsum2_layer_native(tmp_path, flags):
    exe = str(tmp_path / "rowsum2_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "rowsum2_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
