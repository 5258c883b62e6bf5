"""The AEAD open without a GPU (include/tfhe_aes_gpu.h "AEAD open"):

- tae_aead_open_plan against a restatement of the plan, for every accepted tag length and the payload shapes of the edge
  cases;
- the host layer compiled stand-alone (tests/native/aead_open_test.cpp), plain and as a -fsanitize=address,undefined
  binary: padding positions, frame_of_byte, the three truth tables on all their inputs and both plans on plain bits;
- the host model's levels and ids, called in the product library (tests/native/aead_open_noise_test.cpp);
- the schedule check, the refusals and the argument errors; the compute calls without a device.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_var

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PID = tfhe_aes.PARAMS_SQRD_LVL_64
TAG_LENGTHS = (4, 6, 8, 10, 12, 13, 14, 15, 16)  # CCM's 4 .. 16 even, GCM's 4, 8, 12 .. 16


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def plan_restated(tag_len, payload_lens):
    """Level 0 is the 8 tag_len difference bits; every level groups its bits in eights and the levels stop at one bit."""
    groups, bits = [], 8 * tag_len
    while True:
        groups.append(-(-bits // 8))
        if groups[-1] == 1:
            return tuple(groups), sum(payload_lens)
        bits = groups[-1]


@pytest.mark.parametrize("payload_lens", ([0], [1], [17, 0, 3]), ids=("empty", "one", "three"))
@pytest.mark.parametrize("tag_len", TAG_LENGTHS)
def test_plan(tag_len, payload_lens):
    assert aes_var.aead_open_plan(tag_len, payload_lens) == plan_restated(tag_len, payload_lens)


def test_plan_figures():
    want = {4: (4, 1), 8: (8, 1), 12: (12, 2, 1), 13: (13, 2, 1), 16: (16, 2, 1)}
    for tag_len, groups in want.items():
        assert aes_var.aead_open_plan(tag_len, [17, 0, 3]) == (groups, 20)
    assert aes_var.AEAD_TAG_LENGTHS == TAG_LENGTHS
    assert aes_var.aead_open_plan(16, []) == ((16, 2, 1), 0)


def test_plan_refusals():
    for t in (-1, 0, 3, 5, 7, 9, 11, 17, 32):
        assert _code(lambda: aes_var.aead_open_plan(t, [1])) == N.TAE_E_PARAM
    L = N.lib()
    lens = np.array([1], dtype=np.uintp)
    levels, gate = C.c_int(0), C.c_size_t(0)
    groups = np.zeros(3, dtype=np.uintp)
    assert L.tae_aead_open_plan(16, None, 1, C.byref(levels), _vp(groups), C.byref(gate)) == N.TAE_E_ARG
    assert L.tae_aead_open_plan(16, _vp(lens), 1, None, _vp(groups), C.byref(gate)) == N.TAE_E_ARG
    assert L.tae_aead_open_plan(16, _vp(lens), 1, C.byref(levels), None, C.byref(gate)) == N.TAE_E_ARG
    assert L.tae_aead_open_plan(16, _vp(lens), 1, C.byref(levels), _vp(groups), None) == N.TAE_E_ARG


def test_noise_schedule_check():
    cap = tfhe_aes.get_params(PID)["max_noise_sq"]
    assert cap == 64
    for t in TAG_LENGTHS:
        aes_var.aead_open_noise_schedule_check(PID, t)  # a CTR payload bit (9), a CCM difference bit (16)
        aes_var.aead_open_noise_schedule_check(PID, t, cap, cap)
        assert _code(lambda: aes_var.aead_open_noise_schedule_check(PID, t, cap + 1, 1)) == N.TAE_E_NOISE
        assert _code(lambda: aes_var.aead_open_noise_schedule_check(PID, t, 1, cap + 1)) == N.TAE_E_NOISE
    aes_var.aead_open_noise_schedule_check(tfhe_aes.PARAMS_SQRD_LVL_256, 16, 9, 256)
    # a verdict-level output is at 8: above the caps of the two smallest sets
    for pid in (tfhe_aes.PARAMS_SQRD_LVL_1, tfhe_aes.PARAMS_SQRD_LVL_4):
        assert _code(lambda: aes_var.aead_open_noise_schedule_check(pid, 16, 1, 1)) == N.TAE_E_NOISE
    for pid in (tfhe_aes.PARAMS_WOPPBS_8BIT, tfhe_aes.PARAMS_SHORTINT_1BIT, 99):
        assert _code(lambda: aes_var.aead_open_noise_schedule_check(pid, 16)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.aead_open_noise_schedule_check(PID, 5)) == N.TAE_E_PARAM


def test_argument_errors_and_no_device():
    """Null arrays are TAE_E_ARG and a tag length outside the modes' set TAE_E_PARAM, both before the device is looked
    for; then a machine without a GPU answers TAE_E_NODEV (it has no context to pass) and one with a GPU rejects the
    null context."""
    L = N.lib()
    no_context = N.TAE_E_NODEV if tfhe_aes.device_count() == 0 else N.TAE_E_ARG
    a = np.zeros((128, 4), dtype=np.uint64)
    lens = np.array([1], dtype=np.uintp)
    H = N.TAE_MEM_HOST
    assert L.tae_aead_verdict_raw(None, None, 1, 16, _vp(a), H) == N.TAE_E_ARG
    assert L.tae_aead_verdict_raw(None, _vp(a), 1, 16, None, H) == N.TAE_E_ARG
    assert L.tae_aead_verdict_raw(None, _vp(a), 1, 5, _vp(a), H) == N.TAE_E_PARAM
    assert L.tae_aead_verdict_raw(None, _vp(a), 1, 16, _vp(a), H) == no_context
    assert L.tae_aead_open_raw(None, _vp(a), None, _vp(a), 1, 16, _vp(a), _vp(a), H) == N.TAE_E_ARG
    assert L.tae_aead_open_raw(None, None, _vp(lens), _vp(a), 1, 16, _vp(a), _vp(a), H) == N.TAE_E_ARG
    assert L.tae_aead_open_raw(None, _vp(a), _vp(lens), None, 1, 16, _vp(a), _vp(a), H) == N.TAE_E_ARG
    assert L.tae_aead_open_raw(None, _vp(a), _vp(lens), _vp(a), 1, 16, None, _vp(a), H) == N.TAE_E_ARG
    assert L.tae_aead_open_raw(None, _vp(a), _vp(lens), _vp(a), 1, 16, _vp(a), None, H) == N.TAE_E_ARG
    assert L.tae_aead_open_raw(None, _vp(a), _vp(lens), _vp(a), 1, 17, _vp(a), _vp(a), H) == N.TAE_E_PARAM
    assert L.tae_aead_open_raw(None, _vp(a), _vp(lens), _vp(a), 1, 16, _vp(a), _vp(a), H) == no_context
    # a call of no payload needs no payload arrays
    zero = np.array([0], dtype=np.uintp)
    assert L.tae_aead_open_raw(None, None, _vp(zero), _vp(a), 1, 16, None, _vp(a), H) == no_context
    outs = (C.c_void_p * 8)()
    assert L.tae_aead_open(None, None, _vp(lens), outs, 1, 16, outs, outs) == N.TAE_E_ARG
    assert L.tae_aead_open(None, outs, _vp(lens), outs, 1, 16, outs, None) == N.TAE_E_ARG
    assert L.tae_aead_open(None, outs, _vp(lens), outs, 1, 7, outs, outs) == N.TAE_E_PARAM


# ---- the host layer, compiled stand-alone -----------------------------------------------------------------------
@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_open_layer_native(tmp_path, flags):
    exe = str(tmp_path / "aead_open_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "aead_open_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_noise_levels_and_ids_native(tmp_path):
    exe = str(tmp_path / "aead_open_noise_test")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tfhe-aes-2_amd")], check=True)
    lib = os.path.join(ROOT, "tfhe-aes-2_amd", "tfhe_aes")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "aead_open_noise_test.cpp"),
                    os.path.join(lib, "libtfhe_aes_amd.so"), "-o", exe, "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
