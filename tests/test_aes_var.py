"""AES-192 / AES-256 without a GPU: the plain helpers of tfhe_aes.aes_var against FIPS-197 (appendix C.2, C.3)
and against aes_128's helpers at 16-byte keys, the host program for the generalised plain key schedule
(tests/native/aes_var_test.cpp, plain and with sanitizers), and the noise bookkeeping and argument errors of
tae_aesx_noise_schedule_check / tae_aesx_expanded_words.
"""
import os
import random
import subprocess

import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var
from tests.conftest import PKG, ROOT

FIPS_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
FIPS = {16: "69c4e0d86a7b0430d8cdb78070b4c55a",   # C.1
        24: "dda97ca4864cdfe06eaf70a0ec0d7191",   # C.2
        32: "8ea2b7ca516745bfeafc49904b496089"}   # C.3


# ---------------------------------------------------------------- plain helpers ----
@pytest.mark.parametrize("n", [16, 24, 32])
def test_fips197_appendix_c(n):
    key = bytes(range(n))
    ek = aes_var.key_schedule_plain(key)
    assert len(ek) == 4 * (n // 4 + 7) and b"".join(ek[:n // 4]) == key
    assert aes_var.rounds(key) == aes_var.rounds(ek) == n // 4 + 6
    ct = bytes.fromhex(FIPS[n])
    assert aes_var.encrypt_block_plain(ek, FIPS_PT) == ct
    assert aes_var.decrypt_block_plain(ek, ct) == FIPS_PT


def test_fips197_appendix_a_words():
    ek = aes_var.key_schedule_plain(bytes.fromhex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b"))
    assert (ek[6].hex(), ek[7].hex(), ek[51].hex()) == ("fe0c91f7", "2402f5a5", "01002202")
    ek = aes_var.key_schedule_plain(bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"))
    # w8: RotWord, SubWord and Rcon; w12: SubWord alone; w13: plain XOR
    assert (ek[8].hex(), ek[12].hex(), ek[13].hex(), ek[59].hex()) == ("9ba35411", "a8b09c1a", "93d194cd", "706c631e")


def test_16_byte_keys_equal_aes_128_helpers():
    rng = random.Random(197)
    for _ in range(8):
        key, block, iv8, iv16 = (bytes(rng.randrange(256) for _ in range(n)) for n in (16, 16, 8, 16))
        ek = aes_var.key_schedule_plain(key)
        assert ek == aes_128.key_schedule_plain(key)
        assert aes_var.decrypt_key_plain(ek) == aes_128.decrypt_key_plain(ek)
        for r in (1, 2, 10):
            ct = aes_var.encrypt_block_plain(ek, block, r)
            assert ct == aes_128.encrypt_block_plain(ek, block, r)
            assert aes_var.decrypt_block_plain(ek, ct, r) == aes_128.decrypt_block_plain(ek, ct, r) == block
        msg = bytes(rng.randrange(256) for _ in range(48))
        assert aes_var.ctr_xor_plain(key, iv8, 254, msg[:37]) == aes_128.ctr_xor_plain(key, iv8, 254, msg[:37])
        assert aes_var.cbc_encrypt_plain(key, iv16, msg) == aes_128.cbc_encrypt_plain(key, iv16, msg)
        assert aes_var.cbc_decrypt_plain(key, iv16, msg) == aes_128.cbc_decrypt_plain(key, iv16, msg)


def _xtime(a):
    return ((a << 1) ^ (0x1B if a & 0x80 else 0)) & 0xFF


def _mul(a, k):  # by repeated xtime, independent of aes_128.gf_mul
    r = 0
    while k:
        if k & 1:
            r ^= a
        a, k = _xtime(a), k >> 1
    return r


def _mix(col):  # MixColumns of one column
    return bytes(_mul(col[r], 2) ^ _mul(col[(r + 1) % 4], 3) ^ col[(r + 2) % 4] ^ col[(r + 3) % 4] for r in range(4))


@pytest.mark.parametrize("n", [16, 24, 32])
def test_decrypt_key_plain_round_trips(n):
    ek = aes_var.key_schedule_plain(bytes(range(100, 100 + n)))
    dk = aes_var.decrypt_key_plain(ek)
    nr = n // 4 + 6
    assert len(dk) == len(ek) and dk[:4] == ek[:4] and dk[4 * nr:] == ek[4 * nr:]
    assert [_mix(w) for w in dk[4:4 * nr]] == ek[4:4 * nr]  # MixColumns undoes the derivation
    assert all(a != b for a, b in zip(dk[4:4 * nr], ek[4:4 * nr]))


@pytest.mark.parametrize("n", [24, 32])
def test_partial_rounds_ctr_and_cbc_round_trip(n):
    key = bytes((7 * i + 1) & 255 for i in range(n))
    ek = aes_var.key_schedule_plain(key)
    nr = n // 4 + 6
    for r in (1, 2, nr - 1, nr):
        assert aes_var.decrypt_block_plain(ek, aes_var.encrypt_block_plain(ek, FIPS_PT, r), r) == FIPS_PT
    assert aes_var.encrypt_block_plain(ek, FIPS_PT, nr) == aes_var.encrypt_block_plain(ek, FIPS_PT)
    # two rounds read round keys 0, 1 and Nr only: the 128-bit helper on those words gives the same
    ek44 = ek[:40] + ek[-4:]
    assert aes_var.encrypt_block_plain(ek, FIPS_PT, 2) == aes_128.encrypt_block_plain(ek44, FIPS_PT, 2)
    iv8, iv16 = bytes(range(8)), bytes(range(16, 32))
    msg = bytes((29 * i + 7) & 255 for i in range(48))
    ct = aes_var.ctr_xor_plain(key, iv8, 255, msg[:37])  # not a multiple of 16; counters 255, 256, 257
    assert len(ct) == 37 and ct != msg[:37] and aes_var.ctr_xor_plain(key, iv8, 255, ct) == msg[:37]
    assert ct[:16] == bytes(a ^ b for a, b in zip(msg, aes_var.encrypt_block_plain(ek, iv8 + (255).to_bytes(8, "big"))))
    cbc = aes_var.cbc_encrypt_plain(key, iv16, msg)
    assert cbc[:16] == aes_var.encrypt_block_plain(ek, bytes(a ^ b for a, b in zip(msg[:16], iv16)))
    assert aes_var.cbc_decrypt_plain(key, iv16, cbc) == msg
    with pytest.raises(ValueError):
        aes_var.cbc_decrypt_plain(key, iv16, cbc[:17])
    with pytest.raises(ValueError):
        aes_var.key_schedule_plain(key[:20])


# ---------------------------------------------------------------- native program ----
def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra,
                    os.path.join(ROOT, "tests", "native", "aes_var_test.cpp"),
                    os.path.join(PKG, "csrc", "aes_plain.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_native_plain_key_schedule(tmp_path):
    """The host plain_key_schedule at Nk = 4, 6, 8 and a plain cipher over it against FIPS-197 C.1 - C.3."""
    _build_and_run(tmp_path, "aes_var_test", [])


def test_native_plain_key_schedule_sanitized(tmp_path):
    """The same stand-alone program under the address and undefined-behaviour sanitizers: the expansion writes
    into buffers of exactly 16 (Nr + 1) bytes."""
    _build_and_run(tmp_path, "aes_var_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


# ---------------------------------------------------------------- noise and arguments ----
def _x(param_set, key_bits, rounds, inverse):
    try:
        aes_var.noise_schedule_check(param_set, key_bits, rounds, inverse)
        return None
    except tfhe_aes.TaeError as e:
        return e.code


def _128(param_set, rounds, inverse):
    try:
        if inverse:
            aes_128.decrypt_noise_schedule_check(param_set, rounds)
        else:
            aes_128.noise_schedule_check(param_set, N.TAE_DRIVER_GAL_MUL, rounds)
        return None
    except tfhe_aes.TaeError as e:
        return e.code


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("key_bits", [128, 192, 256])
def test_noise_schedule_passes_at_lvl_64(key_bits, inverse):
    nr = key_bits // 32 + 6
    for rounds in range(1, nr + 1):
        assert _x(N.PARAMS_SQRD_LVL_64, key_bits, rounds, inverse) is None, rounds
    assert _x(N.PARAMS_SQRD_LVL_64, key_bits, nr + 1, inverse) == N.TAE_E_PARAM
    assert _x(N.PARAMS_SQRD_LVL_64, key_bits, 0, inverse) == N.TAE_E_PARAM


@pytest.mark.parametrize("param_set", [N.PARAMS_SQRD_LVL_1, N.PARAMS_SQRD_LVL_4, N.PARAMS_SQRD_LVL_64,
                                       N.PARAMS_SQRD_LVL_256])
@pytest.mark.parametrize("inverse", [False, True])
def test_noise_schedule_fails_where_the_128_bit_checks_fail(param_set, inverse):
    """A middle round is 33 and the output 9 at every key size, so the verdict is the 128-bit one: TAE_E_NOISE on
    the two small sets, a pass on the two large ones."""
    max_sq = tfhe_aes.get_params(param_set)["max_noise_sq"]
    for key_bits in (128, 192, 256):
        nr = key_bits // 32 + 6
        for rounds in (1, 2, nr):
            want = _128(param_set, min(rounds, 10), inverse)
            assert _x(param_set, key_bits, rounds, inverse) == want, (key_bits, rounds)
            assert want == (None if max_sq >= 33 else N.TAE_E_NOISE)


def test_argument_errors_and_expanded_words():
    assert [aes_var.expanded_words(kb) for kb in (128, 192, 256)] == [44, 52, 60]
    for bad in (160, 0, 512):
        with pytest.raises(tfhe_aes.TaeError) as e:
            aes_var.expanded_words(bad)
        assert e.value.code == N.TAE_E_PARAM
        for inverse in (False, True):
            assert _x(N.PARAMS_SQRD_LVL_64, bad, 1, inverse) == N.TAE_E_PARAM
    assert _x(N.PARAMS_SQRD_LVL_64, 256, 15, False) == N.TAE_E_PARAM
    assert _x(N.PARAMS_SQRD_LVL_64, 192, 13, True) == N.TAE_E_PARAM
    assert _x(99, 256, 1, False) is not None
    for param_set in (N.PARAMS_WOPPBS_8BIT, N.PARAMS_SHORTINT_1BIT):  # 192 / 256 are the 1-bit model's
        for kb in (192, 256):
            assert _x(param_set, kb, 1, False) == _x(param_set, kb, 1, True) == N.TAE_E_PARAM


def test_key_size_is_read_from_the_key():
    """The Python class refuses keys that are no 44 / 52 / 60 words, and an explicit key_bits that does not match,
    before any native call (the handle arrays are read at the length key_bits implies)."""
    import numpy as np
    V = aes_var.GalMulAes
    blocks = np.zeros((1, 128, 8), dtype=np.uint64)
    for call in (lambda: V.encrypt_blocks_raw(None, np.zeros((52 * 32, 8), dtype=np.uint64), blocks, 1, key_bits=256),
                 lambda: V.decrypt_key_raw(None, np.zeros((51 * 32, 8), dtype=np.uint64)),
                 lambda: V.key_schedule_raw(None, np.zeros((160, 8), dtype=np.uint64)),
                 lambda: V.encrypt_blocks(None, [], [], 1),
                 lambda: V.key_schedule(None, [])):
        with pytest.raises(tfhe_aes.TaeError) as e:
            call()
        assert e.value.code == N.TAE_E_ARG
