"""AES-GCM over key tables without a GPU (include/tfhe_aes_gpu.h "GCM over key tables").

The frames of tae_aesm_gcm_transcipher* are validated on the host before the context is looked at, so the refusals that
depend on the frames alone are checked here with a null context: a slot outside the table, more hashed blocks than
n_powers, a frame shorter than the call's tag (the C-ABI has one tag_len per call, so frames of two tag lengths can only
meet as a frame that does not hold the call's), a bad tag length, a bad IV.  The parameter-set refusal needs a context
and is in tests/test_gpu_gcm_multi.py; mixed tag lengths at the plan level are in tests/native/rowsum2_test.cpp.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_multi
from tests import gcm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 32
NEW = ("tae_aesm_ghash_key_raw", "tae_aesm_ghash_key", "tae_aesm_gcm_transcipher_raw", "tae_aesm_gcm_transcipher")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(streams, n_keys=3, n_powers=4, tag_len=12, rounds=2, key_bits=128):
    """tae_aesm_gcm_transcipher_raw with a null context and dummy arrays: the code and the message."""
    L = N.lib()
    buf = np.zeros((8, 4), dtype=np.uint64)
    arr, _keep, _ = aes_multi._gcm_streams(streams, tag_len)
    code = L.tae_aesm_gcm_transcipher_raw(None, key_bits, _vp(buf), n_keys, _vp(buf), n_powers, arr, len(streams), tag_len,
                                          rounds, _vp(buf), _vp(buf), N.TAE_MEM_HOST)
    return code, L.tae_last_error().decode()


def _handles(streams, n_keys=3, n_powers=4, tag_len=12):
    L = N.lib()
    ptrs = (C.c_void_p * 8)()
    arr, _keep, _ = aes_multi._gcm_streams(streams, tag_len)
    code = L.tae_aesm_gcm_transcipher(None, 128, ptrs, n_keys, ptrs, n_powers, arr, len(streams), tag_len, 2, ptrs, ptrs)
    return code, L.tae_last_error().decode()


GOOD = (2, R.IV3, bytes(8), bytes(20 + 12))  # m = 4


def test_symbols_in_header_and_exported():
    header = open(os.path.join(ROOT, "include", "tfhe_aes_gpu.h")).read()
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in N.EXPORTED and hasattr(lib, name)
    assert "tae_gcm_stream;" in header
    assert [f for f, _ in N.TaeGcmStream._fields_] == ["key", "iv", "iv_len", "aad", "aad_len", "data", "len"]


@pytest.mark.parametrize("call", (_raw, _handles), ids=("raw", "handles"))
def test_frame_refusals_need_no_device(call):
    # a whole call gets as far as the context: no device here, or a null context there
    code, msg = call([GOOD, (0, R.IV3, b"", bytes(12))])
    assert code in (N.TAE_E_NODEV, N.TAE_E_ARG) and "slot" not in msg
    # a slot outside 0 .. n_keys - 1, either side
    for slot in (3, -1, 1 << 20):
        code, msg = call([GOOD, (slot, R.IV3, b"", bytes(12))])
        assert code == N.TAE_E_ARG and "slot" in msg
    code, msg = call([(0, R.IV3, b"", bytes(12))], n_keys=0)
    assert code == N.TAE_E_ARG and "slot" in msg
    # m = 4 > n_powers = 3; m = 5 > 4
    assert call([GOOD], n_powers=3)[0] == N.TAE_E_PARAM
    assert "powers" in call([GOOD], n_powers=3)[1]
    assert call([(0, R.IV3, bytes(17), bytes(20 + 12))])[0] == N.TAE_E_PARAM
    assert call([GOOD], n_powers=65)[0] == N.TAE_E_PARAM and call([GOOD], n_powers=0)[0] == N.TAE_E_PARAM
    # one tag length per call: a frame that holds an 8-byte tag alone in a call of 12
    assert call([GOOD, (1, R.IV3, b"", bytes(8))])[0] == N.TAE_E_PARAM
    for t in (0, 5, 17):
        assert call([(0, R.IV3, b"", bytes(32))], tag_len=t)[0] == N.TAE_E_PARAM
    assert call([(0, bytes(16), b"", bytes(12))])[0] == N.TAE_E_PARAM  # only 96-bit IVs
    # 100 dense hashed blocks: a row beyond 64 chunks, whatever the table holds
    code, _ = call([(0, R.IV3, b"", bytes([0xA5]) * (99 * 16) + bytes(12))], n_powers=64)
    assert code == N.TAE_E_PARAM  # m = 100 > 64 comes first
    assert call([], n_keys=0)[0] in (N.TAE_OK, N.TAE_E_NODEV, N.TAE_E_ARG)


def test_argument_errors():
    L = N.lib()
    buf = np.zeros((8, 4), dtype=np.uint64)
    arr, _keep, _ = aes_multi._gcm_streams([GOOD], 12)
    assert _raw([GOOD], key_bits=160)[0] == N.TAE_E_PARAM
    assert L.tae_aesm_gcm_transcipher_raw(None, 128, None, 3, _vp(buf), 4, arr, 1, 12, 2, _vp(buf), _vp(buf),
                                          N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesm_gcm_transcipher_raw(None, 128, _vp(buf), 3, _vp(buf), 4, None, 1, 12, 2, _vp(buf), _vp(buf),
                                          N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesm_ghash_key_raw(None, 128, None, 2, 4, 2, _vp(buf), N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesm_ghash_key_raw(None, 160, _vp(buf), 2, 4, 2, _vp(buf), N.TAE_MEM_HOST) == N.TAE_E_PARAM
    assert L.tae_aesm_ghash_key(None, 160, (C.c_void_p * 8)(), 2, 4, 2, (C.c_void_p * 8)()) == N.TAE_E_PARAM
    # the Python layer: shapes of the two tables
    table = np.zeros((2, 44 * W, 4), dtype=np.uint64)
    with pytest.raises(tfhe_aes.TaeError) as e:
        aes_multi.GalMulAesMulti.gcm_transcipher_raw(None, table, np.zeros((3, 4, 128, 4), dtype=np.uint64), [GOOD], 12)
    assert e.value.code == N.TAE_E_ARG
