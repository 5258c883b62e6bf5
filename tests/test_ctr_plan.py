"""Counter-mode convention and the round-1 plan (host only, no GPU).

Counter block i is iv || be64(first_counter + i) (main.rs:108-115).  tae_aes_ctr_plan counts the distinct
(byte position, byte value) pairs of a range: the round-1 SBOX groups the counter-mode entry points
bootstrap instead of 16 per block.
"""
import os
import subprocess

import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tfhe_aes import distributed as D
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def readme(golden):
    g = golden["readme_ctr"]
    return bytes.fromhex(g["key"]), bytes.fromhex(g["iv"]), g


@pytest.mark.parametrize("first, n_blocks, groups", [
    (1, 128, 143),      # 8 iv + 7 constant counter bytes + 128 values of byte 15
    (1, 1024, 275),     # 8 + 6 + 5 values of byte 14 (0..4) + 256
    (0xFE, 3, 19),      # 0xFE, 0xFF, 0x100: the carry into byte 14 -> 8 + 6 + 2 + 3
    (897, 128, 144),    # rank 7 of 8: 0x381..0x400 -> byte 14 takes 3 and 4
    (1, 1, 16),
])
def test_ctr_plan_group_counts(readme, first, n_blocks, groups):
    _, iv, _ = readme
    assert aes_128.ctr_plan(iv, first, n_blocks) == groups
    # the count is the number of distinct (position, byte) pairs of the blocks
    blocks = aes_128.counter_blocks(iv, n_blocks, first=first)
    assert len({(pos, blk[pos]) for blk in blocks for pos in range(16)}) == groups


def test_ctr_plan_empty_and_last_counter(readme):
    _, iv, _ = readme
    assert aes_128.ctr_plan(iv, 5, 0) == 0
    assert aes_128.ctr_plan(iv, 2**64 - 1, 1) == 16
    assert aes_128.ctr_plan(iv, 2**64 - 2, 2) == 17


def test_ctr_plan_wrap_is_arg_error(readme):
    _, iv, _ = readme
    with pytest.raises(tfhe_aes.TaeError) as e:
        aes_128.ctr_plan(iv, 2**64 - 1, 2)
    assert e.value.code == N.TAE_E_ARG


def test_counter_blocks_first(readme):
    _, iv, _ = readme
    assert aes_128.counter_blocks(iv, 3, first=0xFE) == [
        iv + bytes.fromhex("00000000000000fe"), iv + bytes.fromhex("00000000000000ff"),
        iv + bytes.fromhex("0000000000000100")]
    assert aes_128.counter_blocks(iv, 2) == aes_128.counter_blocks(iv, 2, first=1)
    assert aes_128.counter_blocks(iv, 2)[0] == iv + (1).to_bytes(8, "big")


@pytest.mark.parametrize("world, per_rank, first", [(8, 128, 1), (2, 3, 0xFE), (1, 5, 7)])
def test_shard_counter_range_matches_shard_counters(world, per_rank, first):
    for rank in range(world):
        start, n = D.shard_counter_range(rank, world, per_rank, first=first)
        assert list(range(start, start + n)) == list(D.shard_counters(rank, world, per_rank, first=first))
    assert D.shard_counter_range(7, 8, 128) == (897, 128)
    with pytest.raises(ValueError):
        D.shard_counter_range(8, 8, 128)


def test_ctr_xor_plain_readme(readme):
    key, iv, g = readme
    want = b"".join(bytes.fromhex(g["ciphertexts"][str(c)]) for c in range(1, 11))
    assert aes_128.ctr_xor_plain(key, iv, 1, bytes(160)) == want
    # a later start, a length that is no multiple of 16, and the round trip
    assert aes_128.ctr_xor_plain(key, iv, 3, bytes(37)) == want[32:69]
    msg = bytes(range(37))
    ct = aes_128.ctr_xor_plain(key, iv, 1, msg)
    assert ct == bytes(m ^ k for m, k in zip(msg, want)) and aes_128.ctr_xor_plain(key, iv, 1, ct) == msg
    assert aes_128.ctr_xor_plain(key, iv, 1, b"") == b""


def test_ctr_plan_groups_and_map(tmp_path):
    """The plan itself (csrc/ctr_plan.hpp; the C-ABI exports only its group count): group list order and
    the (block, position) -> group map, compiled for the host (tests/native/ctr_plan_test.cpp)."""
    exe = str(tmp_path / "ctr_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "ctr_plan_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
