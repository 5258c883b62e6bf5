"""Host-compiled check of the lane-level integer helpers of br512x4's CMux step (fft_device.hpp
torus_add_fast2_sh, rot_diff) against the oracle (or_from_torus, or_decompose) and a naive negacyclic
rotation: tests/native/x4_step_int_test.cpp, CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x4_step_integer_helpers(tmp_path):
    exe = str(tmp_path / "x4_step_int_test")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
                    os.path.join(ROOT, "tests", "native", "x4_step_int_test.cpp"), "-x", "none",
                    os.path.join(ROOT, "oracle", "build", "liboracle.so"), "-o", exe,
                    "-Wl,-rpath," + os.path.join(ROOT, "oracle", "build")], check=True)
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
