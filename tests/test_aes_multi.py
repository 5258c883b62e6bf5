"""Multi-key batches on the host (no GPU): the multi-stream round-1 plan through tae_aesm_ctr_plan, the plan
itself compiled for the host (plain and with the address and undefined-behaviour sanitizers), and the argument
checks that need no device.

A round-1 group is a distinct (slot, byte position, byte value): streams of one slot share groups, streams of
different slots share none.
"""
import os
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_multi
from tests.conftest import ROOT

M = aes_multi.GalMulAesMulti
IV = bytes.fromhex("bdd219b8a08ded1a")
IV2 = bytes(b ^ 0xFF for b in IV)


def _triples(streams):
    """The distinct (slot, position, byte) triples of the streams' counter blocks, computed in Python."""
    out = set()
    for st in streams:
        slot, iv, first = st[:3]
        n = len(st[3]) if st[3] is not None else st[4]
        for blk in aes_128.counter_blocks(iv, (n + 15) // 16, first=first):
            out |= {(slot, pos, blk[pos]) for pos in range(16)}
    return out


@pytest.mark.parametrize("streams, groups", [
    ([(0, IV, 1, bytes(48))], 18),                                   # 8 iv + 7 constant bytes + 3 values of byte 15
    ([(0, IV, 1, bytes(48)), (1, IV, 1, bytes(48))], 36),            # the same public bytes under another key
    ([(0, IV, 1, bytes(48)), (0, IV, 2, bytes(48))], 19),            # 8 + 7 + 4: counters 1..4 of one slot
    ([(0, IV, 1, bytes(48)), (0, IV2, 1, bytes(48))], 26),           # a second iv: its own 8 groups at 0..7
    ([(0, IV, 1, bytes(48)), (0, IV, 7, b"")], 18),                  # a stream of len 0 adds nothing
    ([(0, IV, 1, bytes(48)), (3, IV, 7, None, 0)], 18),
    ([(0, IV, 1, None, 33)], 18),                                    # the keystream form, a partial last block
    ([], 0),
    ([(2, IV, 250, bytes(213)), (0, IV2, 1, bytes(192)), (1, IV, 250, bytes(145)), (2, IV, 255, bytes(95))], 83),
])
def test_plan_group_counts(streams, groups):
    assert M.ctr_plan(streams) == groups == len(_triples(streams))


def test_second_iv_shares_no_iv_position():
    a, b = [(0, IV, 1, bytes(48))], [(0, IV2, 1, bytes(48))]
    ta, tb = _triples(a), _triples(b)
    assert not {t for t in ta if t[1] < 8} & {t for t in tb if t[1] < 8}
    assert {t for t in ta if t[1] >= 8} == {t for t in tb if t[1] >= 8}
    assert M.ctr_plan(a + b) == M.ctr_plan(a) + 8


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def test_plan_errors():
    assert _code(lambda: M.ctr_plan([(0, IV, 2**64 - 1, bytes(17))])) == N.TAE_E_ARG      # a range that wraps
    assert _code(lambda: M.ctr_plan([(0, IV, 1, bytes(16)), (0, IV, 2**64 - 2, None, 48)])) == N.TAE_E_ARG
    assert M.ctr_plan([(0, IV, 2**64 - 1, bytes(16))]) == 16                              # the last counter alone
    assert M.ctr_plan([(0, IV, 2**64 - 1, b"")]) == 0                                     # no block, no range
    assert _code(lambda: M.ctr_plan([(-1, IV, 1, bytes(1))])) == N.TAE_E_ARG
    lib = tfhe_aes.lib()
    assert lib.tae_aesm_ctr_plan(None, 0, None) == N.TAE_E_ARG


def test_argument_errors_without_a_device():
    """What the Python class and the C-ABI refuse before any context is touched."""
    L = 8
    blocks = np.zeros((2, 128, L), dtype=np.uint64)
    t44 = np.zeros((2, 44 * 32, L), dtype=np.uint64)
    # a table whose row count is no expanded key, or that is no [n_keys][rows][L] array
    assert _code(lambda: M.encrypt_blocks_raw(None, t44[:, :-32], [0, 1], blocks, 1)) == N.TAE_E_ARG
    assert _code(lambda: M.decrypt_blocks_raw(None, t44[:, :-1], [0, 1], blocks, 1)) == N.TAE_E_ARG
    assert _code(lambda: M.decrypt_key_raw(None, t44[0])) == N.TAE_E_ARG
    assert _code(lambda: M.ctr_transcipher_raw(None, t44[:, :33], [(0, IV, 1, b"a")])) == N.TAE_E_ARG
    assert _code(lambda: M.cbc_transcipher_raw(None, t44[0], [(0, bytes(16), bytes(16))])) == N.TAE_E_ARG
    # one slot per block
    assert _code(lambda: M.encrypt_blocks_raw(None, t44, [0], blocks, 1)) == N.TAE_E_ARG
    # keys of no AES size
    assert _code(lambda: M.key_schedule_raw(None, np.zeros((2, 160, L), dtype=np.uint64))) == N.TAE_E_ARG
    assert _code(lambda: M.key_schedule_raw(None, np.zeros((128, L), dtype=np.uint64))) == N.TAE_E_ARG
    assert _code(lambda: M.key_schedule(None, [[], []])) == N.TAE_E_ARG
    assert M.key_schedule(None, []) == []
    # the C-ABI without a context: null is TAE_E_ARG, never a crash
    lib = tfhe_aes.lib()
    assert lib.tae_aesm_key_schedule_raw(None, 128, None, 0, None, N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert lib.tae_aesm_encrypt_blocks_raw(None, 128, None, 0, None, None, 0, 1, None, N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert lib.tae_aesm_ctr_transcipher_raw(None, 128, None, 0, None, 0, 1, None, N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert lib.tae_aesm_cbc_transcipher_raw(None, 128, None, 0, None, 0, 1, None, N.TAE_MEM_HOST) == N.TAE_E_ARG
    with pytest.raises(ValueError):
        M.ctr_plan([(0, IV[:7], 1, b"a")])
    with pytest.raises(ValueError):
        M.ctr_plan([(0, IV, 1, None)])  # the keystream form needs a length


def test_exports():
    assert tfhe_aes.aes_multi is aes_multi
    for name in ("tae_aesm_key_schedule_raw", "tae_aesm_decrypt_key_raw", "tae_aesm_encrypt_blocks_raw",
                 "tae_aesm_decrypt_blocks_raw", "tae_aesm_ctr_plan", "tae_aesm_ctr_transcipher_raw",
                 "tae_aesm_cbc_transcipher_raw", "tae_aesm_key_schedule", "tae_aesm_ctr_transcipher",
                 "tae_aesm_cbc_transcipher"):
        assert name in N.EXPORTED and hasattr(tfhe_aes.lib(), name)


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags,
                    os.path.join(ROOT, "tests", "native", "ctr_plan_multi_test.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name, flags", [
    ("plain", []),
    ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]),
])
def test_plan_groups_and_map_native(tmp_path, name, flags):
    """csrc/ctr_plan.hpp compiled for the host as a stand-alone program: groups pairwise distinct, every
    (block, position) mapped to the group of its (slot, position, value), the same group count at every chunk size."""
    r = subprocess.run([_build(tmp_path, "ctr_plan_multi_" + name, flags)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
