"""The AES-128 inverse cipher and CBC transciphering on the GPU (tae_aes_decrypt_*, tae_aes_cbc_*; FIPS-197
5.3, the reference has no decryption).

The circuit bootstrap is deterministic in its input ciphertexts, so the device path must give, word for word,
a Python composition of the algorithm in csrc/aes_inv.hpp: numpy uint64 additions around the CPU oracle's
circuit_bootstrap (8 -> 32 with InvSbox * {14, 11, 13, 9}, 8 -> 8 with InvSbox, 1 -> 1 identity).  The key is
the FIPS-197 C.1 key throughout.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
E = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
KEY = bytes(range(16))
FIPS_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
FIPS_CT = bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a")
MUL = (14, 11, 13, 9)


def f_inv32(x):
    y = aes_128.INV_SBOX[x]
    return (aes_128.gf_mul(y, 14) << 24) | (aes_128.gf_mul(y, 11) << 16) | (aes_128.gf_mul(y, 13) << 8) | aes_128.gf_mul(y, 9)


def f_mul32(x):
    return (aes_128.gf_mul(x, 14) << 24) | (aes_128.gf_mul(x, 11) << 16) | (aes_128.gf_mul(x, 13) << 8) | aes_128.gf_mul(x, 9)


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _trivial_blocks(blocks):
    bits = aes_128.blocks_to_bits(blocks).astype(np.uint64)
    cts = np.zeros((len(blocks), 128, BIG), dtype=np.uint64)
    cts[:, :, -1] = bits << np.uint64(63)
    return cts


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def ek_plain():
    return aes_128.key_schedule_plain(KEY)


@pytest.fixture(scope="module")
def rk(client, ek_plain):
    """Fresh encryption of the plain expanded key [1408][BIG]."""
    return client.encrypt_bits_raw(_bits(b"".join(ek_plain)), start_index=5_000_000)


@pytest.fixture(scope="module")
def dk_fresh(client, ek_plain):
    """Fresh encryption of the PLAIN decryption key: what the word-for-word compositions run on."""
    return client.encrypt_bits_raw(_bits(b"".join(aes_128.decrypt_key_plain(ek_plain))), start_index=5_010_000)


@pytest.fixture(scope="module")
def dk_gpu(gpu_context, rk):
    """The decryption key derived on the device from rk."""
    return E.decrypt_key_raw(gpu_context, rk)


@pytest.fixture(scope="module")
def luts(oracle_mod, oracle_keys):
    n = oracle_keys.p["N"]
    return {"inv32": oracle_mod.generate_lut(n, 8, 32, f_inv32),
            "inv8": oracle_mod.generate_lut(n, 8, 8, lambda x: aes_128.INV_SBOX[x]),
            "mul32": oracle_mod.generate_lut(n, 8, 32, f_mul32),
            "id1": oracle_mod.generate_lut(n, 1, 1, lambda x: x)}


def _cbs_many(oracle_keys, groups, lut, n_out):
    """oracle circuit bootstrap of every group [G][n_in][BIG] -> [G][n_out][BIG] on a pool of 16 threads."""
    with ThreadPoolExecutor(max_workers=16) as pool:
        return np.stack(list(pool.map(lambda g: oracle_keys.circuit_bootstrap(g, lut, n_out), groups)))


def _key_bit(key, word, row, bit):
    return key[(word * 4 + row) * 8 + bit]


def _combine(muls, shift_rows):
    """InvMixColumns (after InvShiftRows when shift_rows) on muls [16][32][BIG] -> [128][BIG]."""
    out = np.zeros((128, BIG), dtype=np.uint64)
    for c in range(4):
        for row in range(4):
            for bit in range(8):
                acc = out[(4 * c + row) * 8 + bit]
                for j in range(4):
                    rr = (row + j) & 3
                    acc += muls[4 * (((c - rr) & 3) if shift_rows else c) + rr][8 * j + bit]
    return out


def _oracle_decrypt_block(oracle_keys, luts, dk, block, rounds):
    state = block + dk[40 * 32:44 * 32]
    for r in range(rounds - 1, 0, -1):
        muls = _cbs_many(oracle_keys, state.reshape(16, 8, BIG), luts["inv32"], 32)
        state = _combine(muls, True) + dk[4 * r * 32:(4 * r + 4) * 32]
    sb = _cbs_many(oracle_keys, state.reshape(16, 8, BIG), luts["inv8"], 8)
    out = np.zeros((128, BIG), dtype=np.uint64)
    for c in range(4):
        for row in range(4):
            for bit in range(8):
                out[(4 * c + row) * 8 + bit] = sb[4 * ((c - row) & 3) + row][bit] + _key_bit(dk, c, row, bit)
    return out


def test_cbs_8_to_32_two_groups_equal_oracle(gpu_context, oracle_keys, client, luts):
    """n_out = 32 is no multiple of the ciphertexts per vertical-packing workgroup, and the second group
    checks the group stride of inputs and outputs."""
    lut = gpu_context.generate_lookup_table(8, 32, f_inv32)
    assert np.array_equal(lut.as_array(), luts["inv32"])
    cts = client.encrypt_bits_raw(_bits(bytes([0x53, 0x00])), start_index=5_020_000).reshape(2, 8, BIG)
    out = gpu_context.circuit_bootstrap_raw(cts, lut)
    assert out.shape == (2, 32, BIG)
    ref = _cbs_many(oracle_keys, cts, luts["inv32"], 32)
    assert np.array_equal(out, ref)
    got = client.decrypt_bits_raw(out).reshape(2, 4, 8)
    for g, x in enumerate((0x53, 0x00)):
        y = aes_128.INV_SBOX[x]
        assert [aes_128.bits_to_u8(b) for b in got[g]] == [aes_128.gf_mul(y, m) for m in MUL]


def test_two_blocks_two_rounds_equal_composition(gpu_context, oracle_keys, client, ek_plain, dk_fresh, luts, golden):
    pts = [bytes.fromhex(golden["chacha20_zero_seed"][b]) for b in ("block1", "block2")]
    cts_plain = [aes_128.encrypt_block_plain(ek_plain, p, 2) for p in pts]
    blocks = client.encrypt_bits_raw(aes_128.blocks_to_bits(cts_plain).reshape(-1), start_index=5_030_000)
    blocks = blocks.reshape(2, 128, BIG)
    out = E.decrypt_blocks_raw(gpu_context, dk_fresh, blocks, rounds=2)
    assert out.shape == (2, 128, BIG)
    assert np.array_equal(out[1], _oracle_decrypt_block(oracle_keys, luts, dk_fresh, blocks[1], 2))
    got = aes_128.bits_to_blocks(client.decrypt_bits_raw(out))
    assert got == [aes_128.decrypt_block_plain(ek_plain, c, 2) for c in cts_plain] == pts


def test_one_round_equals_composition(gpu_context, oracle_keys, client, ek_plain, dk_fresh, luts):
    ct = aes_128.encrypt_block_plain(ek_plain, FIPS_PT, 1)
    block = client.encrypt_bits_raw(aes_128.blocks_to_bits([ct]).reshape(-1), start_index=5_040_000).reshape(1, 128, BIG)
    out = E.decrypt_blocks_raw(gpu_context, dk_fresh, block, rounds=1)
    assert np.array_equal(out[0], _oracle_decrypt_block(oracle_keys, luts, dk_fresh, block[0], 1))
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(out)) == [FIPS_PT]


def test_ten_rounds_two_blocks_with_derived_key(gpu_context, client, ek_plain, dk_gpu, golden):
    other = bytes.fromhex(golden["test_light"]["block1"]["10"])
    blocks = client.encrypt_bits_raw(aes_128.blocks_to_bits([FIPS_CT, other]).reshape(-1), start_index=5_050_000)
    out = E.decrypt_blocks_raw(gpu_context, dk_gpu, blocks.reshape(2, 128, BIG))
    got = aes_128.bits_to_blocks(client.decrypt_bits_raw(out))
    assert got == [FIPS_PT, aes_128.decrypt_block_plain(ek_plain, other)]


def test_raw_round_trip(gpu_context, client, rk, dk_gpu, golden):
    pts = [FIPS_PT, bytes.fromhex(golden["chacha20_zero_seed"]["block2"])]
    x = client.encrypt_bits_raw(aes_128.blocks_to_bits(pts).reshape(-1), start_index=5_060_000).reshape(2, 128, BIG)
    enc = E.encrypt_blocks_raw(gpu_context, rk, x)
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(enc))[0] == FIPS_CT
    back = E.decrypt_blocks_raw(gpu_context, dk_gpu, enc)
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(back)) == pts


def test_handles_key_levels_and_round_trip_is_not_independent(gpu_context, client, ek_plain, rk):
    """decrypt_key on handles: level 1 on words 4..39, the input's bits elsewhere.  One round is enough for
    the independence rule: encrypt_blocks' output already carries round key 10's ids."""
    ek = [gpu_context.bit_from_data(rk[i], 1) for i in range(44 * 32)]
    dk = E.decrypt_key(gpu_context, ek)
    flat = [b for w in dk for byte in w for b in byte]
    assert len(flat) == 44 * 32
    assert {b.noise_level_squared for b in flat[4 * 32:40 * 32]} == {1}
    for i in list(range(0, 128, 17)) + list(range(40 * 32, 44 * 32, 17)):
        assert np.array_equal(flat[i].data(BIG), rk[i])
    want = b"".join(aes_128.decrypt_key_plain(ek_plain))
    assert aes_128.decrypt_byte_array(client, [byte for w in dk[36:40] for byte in w]) == want[144:160]
    block = aes_128.encrypt_byte_array(client, FIPS_PT)
    enc = E.encrypt_block_for_rounds(gpu_context, ek, block, 1)
    with pytest.raises(tfhe_aes.NoiseNotIndependent):
        E.decrypt_block_for_rounds(gpu_context, dk, enc, 1)
    # a fresh encryption of the same ciphertext decrypts, with the schedule's output level 8 + 1
    ct = aes_128.encrypt_block_plain(ek_plain, FIPS_PT, 1)
    assert aes_128.decrypt_byte_array(client, enc) == ct
    out = E.decrypt_block_for_rounds(gpu_context, dk, aes_128.encrypt_byte_array(client, ct), 1)
    assert {b.noise_level_squared for byte in out for b in byte} == {9}
    assert aes_128.decrypt_byte_array(client, out) == FIPS_PT


def test_decrypt_key_derivation(gpu_context, oracle_keys, client, ek_plain, rk, dk_gpu, luts):
    assert dk_gpu.shape == (44 * 32, BIG)
    assert np.array_equal(dk_gpu[:128], rk[:128]) and np.array_equal(dk_gpu[40 * 32:], rk[40 * 32:])
    want = b"".join(aes_128.decrypt_key_plain(ek_plain))
    bits = client.decrypt_bits_raw(dk_gpu).reshape(176, 8)
    assert bytes(aes_128.bits_to_u8(b) for b in bits) == want
    # words 36..39 (round key 9): 16 groups of 8 -> 32, the 4-term sums, 128 identity bootstraps
    muls = _cbs_many(oracle_keys, rk[36 * 32:40 * 32].reshape(16, 8, BIG), luts["mul32"], 32)
    summed = _combine(muls, False)
    ref = _cbs_many(oracle_keys, summed.reshape(128, 1, BIG), luts["id1"], 1).reshape(128, BIG)
    assert np.array_equal(dk_gpu[36 * 32:40 * 32], ref)


def test_cbc_three_blocks(gpu_context, client, dk_gpu):
    torch = pytest.importorskip("torch")
    iv = bytes(range(0xA0, 0xB0))
    msg = bytes((37 * i + 11) & 255 for i in range(48))
    data = aes_128.cbc_encrypt_plain(KEY, iv, msg)  # what the client sends
    out = E.cbc_transcipher_raw(gpu_context, dk_gpu, iv, data)
    assert out.shape == (48, 8, BIG)
    blocks = [data[i:i + 16] for i in (0, 16, 32)]
    want = E.decrypt_blocks_raw(gpu_context, dk_gpu, _trivial_blocks(blocks)).reshape(48, 8, BIG)
    prev = np.array([aes_128.u8_to_bits(b) for b in iv + data[:32]], dtype=np.uint64)
    want[:, :, -1] += prev << np.uint64(63)
    assert np.array_equal(out, want)
    bits = client.decrypt_bits_raw(out).reshape(48, 8)
    assert bytes(aes_128.bits_to_u8(b) for b in bits) == aes_128.cbc_decrypt_plain(KEY, iv, data) == msg
    with pytest.raises(tfhe_aes.TaeError) as e:
        E.cbc_transcipher_raw(gpu_context, dk_gpu, iv, data[:17])
    assert e.value.code == N.TAE_E_ARG
    assert E.cbc_transcipher_raw(gpu_context, dk_gpu, iv, b"").shape == (0, 8, BIG)
    d_dk = torch.from_numpy(dk_gpu.view(np.int64)).to("cuda:0")
    d_out = torch.full((48, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    E.cbc_transcipher_device(gpu_context, d_dk.data_ptr(), iv, data, d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), out)


def test_cbc_handles_one_block(gpu_context, client, rk):
    """The handle variant: the noise level of a decrypt on trivial inputs, and the message."""
    iv = bytes(range(0xA0, 0xB0))
    data = aes_128.cbc_encrypt_plain(KEY, iv, b"sixteen byte msg")
    dk = E.decrypt_key(gpu_context, [gpu_context.bit_from_data(rk[i], 1) for i in range(44 * 32)])
    out = E.cbc_transcipher(gpu_context, dk, iv, data)
    assert len(out) == 16 and {b.noise_level_squared for byte in out for b in byte} == {9}
    assert aes_128.decrypt_byte_array(client, out) == b"sixteen byte msg"
    with pytest.raises(tfhe_aes.TaeError) as e:
        E.cbc_transcipher(gpu_context, dk, iv, data + b"x")
    assert e.value.code == N.TAE_E_ARG
    assert E.cbc_transcipher(gpu_context, dk, iv, b"") == []


def _assert_param_errors(ctx):
    key = np.zeros((44 * 32, ctx.lwe_size), dtype=np.uint64)
    blocks = np.zeros((1, 128, ctx.lwe_size), dtype=np.uint64)
    for call in (lambda: E.decrypt_key_raw(ctx, key), lambda: E.decrypt_blocks_raw(ctx, key, blocks, 1),
                 lambda: E.cbc_transcipher_raw(ctx, key, bytes(16), bytes(16)),
                 lambda: E.decrypt_key(ctx, [ctx.trivial(tfhe_aes.Cleartext(0))] * (44 * 32)),
                 lambda: E.cbc_transcipher(ctx, [ctx.trivial(tfhe_aes.Cleartext(0))] * (44 * 32), bytes(16), bytes(16))):
        with pytest.raises(tfhe_aes.TaeError) as e:
            call()
        assert e.value.code == N.TAE_E_PARAM


def test_8bit_model_is_param_error(gpu_context8):
    _assert_param_errors(gpu_context8)


def test_shortint_1bit_is_param_error():
    P5 = tfhe_aes.PARAMS_SHORTINT_1BIT
    _, keys = tfhe_aes.generate_keys_raw(P5, SEED, threads=16)
    _assert_param_errors(tfhe_aes.context_from_raw(P5, keys, device=0))
