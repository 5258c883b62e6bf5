"""The row-sum layer (csrc/rowsum.hpp) on the host: tests/native/rowsum_test.cpp runs rowsum_word with every nullable
argument both ways against a direct double loop, what rowplan_ok refuses, and a plan repeated through list_of /
base_of against the explicit copy of its lists -- plain and as a -fsanitize=address,undefined binary."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_rowsum_layer_native(tmp_path, flags):
    exe = str(tmp_path / "rowsum_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "rowsum_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
