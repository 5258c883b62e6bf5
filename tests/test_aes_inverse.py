"""The AES-128 inverse cipher without a GPU: the plain helpers (FIPS-197 5.3; the reference has no
decryption), the host program that pins the kernels' tables and indexing (tests/native/aes_inv_test.cpp),
and the noise bookkeeping of the decryption-key derivation and the decrypt rounds
(tae_aes_decrypt_noise_schedule_check) against a Python transcription of the algorithm in csrc/aes_inv.hpp.
"""
import itertools
import os
import subprocess

import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tests.conftest import ROOT

FIPS_KEY = bytes(range(16))
FIPS_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
FIPS_CT = bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a")


# ---------------------------------------------------------------- plain helpers ----
@pytest.mark.parametrize("rounds", [1, 2, 10])
def test_decrypt_block_plain_inverts_encrypt(golden, rounds):
    g = golden["test_light"]
    ek = aes_128.key_schedule_plain(bytes.fromhex(g["key"]))
    assert b"".join(ek).hex() == g["round_keys"]
    for name in ("block1", "block2"):
        pt = bytes.fromhex(golden["chacha20_zero_seed"][name])
        ct = bytes.fromhex(g[name][str(rounds)])
        assert aes_128.encrypt_block_plain(ek, pt, rounds) == ct
        assert aes_128.decrypt_block_plain(ek, ct, rounds) == pt


def test_fips197_c1_round_trip():
    ek = aes_128.key_schedule_plain(FIPS_KEY)
    assert aes_128.encrypt_block_plain(ek, FIPS_PT) == FIPS_CT
    assert aes_128.decrypt_block_plain(ek, FIPS_CT) == FIPS_PT


def test_gf_mul_and_inv_sbox():
    assert aes_128.gf_mul(0x57, 0x83) == 0xC1 and aes_128.gf_mul(0x57, 0x13) == 0xFE  # FIPS-197 4.2, 4.2.1
    assert all(aes_128.INV_SBOX[aes_128.SBOX[x]] == x for x in range(256))
    assert aes_128.INV_SBOX[0x00] == 0x52 and aes_128.INV_SBOX[0xED] == 0x53
    # the reference's quirky gf_256_mul differs from the true product (it is right only inside MixColumns)
    assert aes_128.gf_256_mul(0x57, 2) != aes_128.gf_mul(0x57, 2) == 0xAE


def _xtime(a):
    return ((a << 1) ^ (0x1B if a & 0x80 else 0)) & 0xFF


def _mul(a, k):  # by repeated xtime, independent of aes_128.gf_mul
    r = 0
    while k:
        if k & 1:
            r ^= a
        a, k = _xtime(a), k >> 1
    return r


def test_decrypt_key_plain_is_inv_mix_columns_of_round_keys():
    ek = aes_128.key_schedule_plain(FIPS_KEY)
    dk = aes_128.decrypt_key_plain(ek)
    assert len(dk) == 44 and dk[0:4] == ek[0:4] and dk[40:44] == ek[40:44]
    for w in range(4, 40):
        col = ek[w]
        want = bytes(_mul(col[r], 14) ^ _mul(col[(r + 1) % 4], 11) ^ _mul(col[(r + 2) % 4], 13)
                     ^ _mul(col[(r + 3) % 4], 9) for r in range(4))
        assert dk[w] == want, w
    # FIPS-197 C.1, equivalent inverse cipher: round[9].ik_sch
    assert b"".join(dk[4:8]).hex() == "8c56dff0825dd3f9805ad3fc8659d7fd"


def test_cbc_round_trip_three_blocks(golden):
    key = bytes.fromhex(golden["test_light"]["key"])
    iv = bytes(range(0x10, 0x20))
    msg = bytes((29 * i + 7) & 255 for i in range(48))
    ct = aes_128.cbc_encrypt_plain(key, iv, msg)
    assert len(ct) == 48 and ct != msg
    ek = aes_128.key_schedule_plain(key)
    assert ct[:16] == aes_128.encrypt_block_plain(ek, bytes(a ^ b for a, b in zip(msg[:16], iv)))
    assert ct[16:32] == aes_128.encrypt_block_plain(ek, bytes(a ^ b for a, b in zip(msg[16:32], ct[:16])))
    assert aes_128.cbc_decrypt_plain(key, iv, ct) == msg
    assert aes_128.cbc_decrypt_plain(key, iv, b"") == b""
    with pytest.raises(ValueError):
        aes_128.cbc_decrypt_plain(key, iv, ct[:17])


# ---------------------------------------------------------------- native program ----
def test_native_tables_and_indexing(tmp_path):
    """csrc/aes_inv.hpp on the host, with the address and undefined-behaviour sanitizers: the FIPS vector
    through the muls [16][4] -> combine data flow of the kernels, and the three table functions."""
    exe = str(tmp_path / "aes_inv_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "aes_inv_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


# ---------------------------------------------------------------- noise ----
_ids = itertools.count()


class NoiseLevelWithComponents:
    """shortint_woppbs_1bit.rs:34-78: squared level + the ids of the fresh ciphertexts it is built from."""

    def __init__(self, level, components=()):
        self.level, self.components = level, set(components)

    @classmethod
    def fresh(cls, level):
        return cls(level, {next(_ids)})

    def copy(self):
        return NoiseLevelWithComponents(self.level, self.components)

    def add_assign(self, rhs, max_sq):
        if self.components & rhs.components:
            raise tfhe_aes.NoiseNotIndependent(N.TAE_E_INDEP, "noise components not independent")
        self.components |= rhs.components
        self.level += rhs.level
        if self.level > max_sq:
            raise tfhe_aes.NoiseTooBig(N.TAE_E_NOISE, f"NoiseTooBig {self.level} > {max_sq}")


F = NoiseLevelWithComponents.fresh


def _byte(rr, cc):
    return 4 * cc + rr


def decrypt_key_schedule(rk, max_sq):
    """rk [44][4][8] levels -> dk: one 8 -> 32 bootstrap of the 144 bytes (outputs level 8, fresh ids), the
    4-term sum without InvShiftRows, one identity bootstrap per bit (level 1, fresh id)."""
    dk = [[[b.copy() for b in byte] for byte in word] for word in rk]
    levels = set()
    for r in range(1, 10):
        muls = [[[F(8) for _ in range(8)] for _ in range(4)] for _ in range(16)]  # [byte][m][bit]
        for c in range(4):
            for row in range(4):
                for bit in range(8):
                    v = muls[_byte(row, c)][0][bit].copy()
                    for j in range(1, 4):
                        v.add_assign(muls[_byte((row + j) & 3, c)][j][bit], max_sq)
                    levels.add(v.level)
                    dk[4 * r + c][row][bit] = F(1)
    return dk, levels


def decrypt_schedule(dk, block, rounds, max_sq):
    """decrypt_block_for_rounds on levels: block [16][8] (pos = 4*col + row); returns the output and the
    levels the state takes after each middle round."""
    state = [[b.copy() for b in byte] for byte in block]
    for c in range(4):
        for row in range(4):
            for bit in range(8):
                state[_byte(row, c)][bit].add_assign(dk[40 + c][row][bit], max_sq)
    round_levels = set()
    for r in range(rounds - 1, 0, -1):
        muls = [[[F(8) for _ in range(8)] for _ in range(4)] for _ in range(16)]
        nxt = [[None] * 8 for _ in range(16)]
        for c in range(4):
            for row in range(4):
                for bit in range(8):
                    v = None
                    for j in range(4):
                        rr = (row + j) & 3
                        t = muls[_byte(rr, (c - rr) & 3)][j][bit]
                        if v is None:
                            v = t.copy()
                        else:
                            v.add_assign(t, max_sq)
                    v.add_assign(dk[4 * r + c][row][bit], max_sq)
                    round_levels.add(v.level)
                    nxt[_byte(row, c)][bit] = v
        state = nxt
    sb = [[F(8) for _ in range(8)] for _ in range(16)]
    out = [[None] * 8 for _ in range(16)]
    for c in range(4):
        for row in range(4):
            for bit in range(8):
                v = sb[_byte(row, (c - row) & 3)][bit].copy()
                v.add_assign(dk[c][row][bit], max_sq)
                out[_byte(row, c)][bit] = v
    return out, round_levels


def _restated(rounds, max_sq):
    rk = [[[F(1) for _ in range(8)] for _ in range(4)] for _ in range(44)]
    block = [[F(1) for _ in range(8)] for _ in range(16)]
    try:
        dk, _ = decrypt_key_schedule(rk, max_sq)
        decrypt_schedule(dk, block, rounds, max_sq)
        return None
    except tfhe_aes.TaeError as e:
        return type(e)


def _product(param_set, rounds):
    try:
        aes_128.decrypt_noise_schedule_check(param_set, rounds)
        return None
    except tfhe_aes.TaeError as e:
        return type(e)


@pytest.mark.parametrize("param_set", [N.PARAMS_SQRD_LVL_1, N.PARAMS_SQRD_LVL_4, N.PARAMS_SQRD_LVL_64,
                                       N.PARAMS_SQRD_LVL_256])
@pytest.mark.parametrize("rounds", [1, 2, 10])
def test_decrypt_noise_schedule_matches_restatement(param_set, rounds):
    max_sq = tfhe_aes.get_params(param_set)["max_noise_sq"]
    want = _restated(rounds, max_sq)
    assert _product(param_set, rounds) is want
    # the key derivation's 4-term sum alone needs 32: the two small sets fail on noise, never on independence
    assert want is (None if max_sq >= 33 else tfhe_aes.NoiseTooBig)


def test_levels_at_lvl_64():
    max_sq = tfhe_aes.get_params(N.PARAMS_SQRD_LVL_64)["max_noise_sq"]
    assert max_sq == 64
    rk = [[[F(1) for _ in range(8)] for _ in range(4)] for _ in range(44)]
    dk, combine = decrypt_key_schedule(rk, max_sq)
    assert combine == {32}
    assert {b.level for w in dk[4:40] for byte in w for b in byte} == {1}
    block = [[F(1) for _ in range(8)] for _ in range(16)]
    out, rounds_ = decrypt_schedule(dk, block, 10, max_sq)
    assert rounds_ == {33} and {b.level for byte in out for b in byte} == {9}
    out1, rounds1 = decrypt_schedule(dk, block, 1, max_sq)
    assert rounds1 == set() and {b.level for byte in out1 for b in byte} == {9}


def test_reused_round_key_10_breaks_independence():
    """encrypt_blocks' output carries the ids of round key 10; the decryption key's words 40..43 are that
    round key, so the first XOR of a decrypt of that output must raise."""
    rk = [[[F(1) for _ in range(8)] for _ in range(4)] for _ in range(44)]
    dk, _ = decrypt_key_schedule(rk, 64)
    enc_out = [[None] * 8 for _ in range(16)]
    for c in range(4):
        for row in range(4):
            for bit in range(8):
                v = F(8)
                v.add_assign(rk[40 + c][row][bit], 64)
                enc_out[_byte(row, c)][bit] = v
    with pytest.raises(tfhe_aes.NoiseNotIndependent):
        decrypt_schedule(dk, enc_out, 10, 64)


@pytest.mark.parametrize("param_set", [N.PARAMS_WOPPBS_8BIT, N.PARAMS_SHORTINT_1BIT])
def test_other_models_are_param_errors(param_set):
    with pytest.raises(tfhe_aes.TaeError) as e:
        aes_128.decrypt_noise_schedule_check(param_set, 10)
    assert e.value.code == N.TAE_E_PARAM


def test_schedule_check_arguments():
    for rounds in (0, 11):
        with pytest.raises(tfhe_aes.TaeError) as e:
            aes_128.decrypt_noise_schedule_check(N.PARAMS_SQRD_LVL_64, rounds)
        assert e.value.code == N.TAE_E_PARAM
    with pytest.raises(tfhe_aes.TaeError):
        aes_128.decrypt_noise_schedule_check(99, 1)


def test_other_driver_classes_refuse():
    """The 1-bit fhe_sbox_pbs driver and the classes of the other models raise before any native call."""
    for cls in (aes_128.ShortintWoppbs1BitSboxPbsAesEncrypt, aes_128.ShortintWoppbs8BitSboxPbsAesEncrypt,
                aes_128.Shortint1BitSboxPbsAesEncrypt):
        for call in (lambda: cls.decrypt_key(None, []), lambda: cls.decrypt_blocks(None, [], [], 1),
                     lambda: cls.decrypt_key_raw(None, None), lambda: cls.decrypt_blocks_raw(None, None, None),
                     lambda: cls.decrypt_blocks_device(None, 0, 0, 0, 1, 0),
                     lambda: cls.cbc_transcipher(None, [], bytes(16), b""),
                     lambda: cls.cbc_transcipher_raw(None, None, bytes(16), b""),
                     lambda: cls.decrypt_block(None, [], []),
                     lambda: cls.decrypt_block_for_rounds(None, [], [], 2)):
            with pytest.raises(tfhe_aes.TaeError) as e:
                call()
            assert e.value.code == N.TAE_E_PARAM
