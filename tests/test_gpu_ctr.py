"""AES-128-CTR with public counters on the GPU (tae_aes_ctr_*): no counter ciphertexts, round 1 bootstrapped
once per distinct (byte position, byte value) pair and read through the plan's map.

The circuit bootstrap is deterministic in its input ciphertexts, so the deduplicated path must give the
words the per-block entry points give on TRIVIAL encryptions of the counter blocks (zero mask, bit << 63 on
the body), which in turn equal the CPU oracle.  first_counter = 0xFE with 3 blocks is the smallest shape
with shared groups (the iv, counter bytes 8..13), three distinct values in byte 15 and a carry into byte
14 (19 groups instead of 48).
"""
import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
SMALL = 786
E = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
A8 = aes_128.ShortintWoppbs8BitSboxPbsAesEncrypt
V = aes_var.GalMulAes  # the entry points that take `rounds` where the AES-128 ones run all ten
CARRY_FIRST, CARRY_BLOCKS = 0xFE, 3


def _trivial_blocks(blocks, lwe_size):
    """Trivial encryptions of the blocks' bits: [n][128][lwe_size], zero mask, bit << 63 on the body."""
    bits = aes_128.blocks_to_bits(blocks).astype(np.uint64)
    cts = np.zeros((len(blocks), 128, lwe_size), dtype=np.uint64)
    cts[:, :, -1] = bits << np.uint64(63)
    return cts


def _expanded_key_bits(key):
    ek = b"".join(aes_128.key_schedule_plain(key))
    return [b for byte in ek for b in aes_128.u8_to_bits(byte)]


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def readme_setup(client, golden):
    g = golden["readme_ctr"]
    key, iv = bytes.fromhex(g["key"]), bytes.fromhex(g["iv"])
    rk = client.encrypt_bits_raw(_expanded_key_bits(key), start_index=300_000)
    return key, iv, rk


@pytest.fixture(scope="module")
def carry_case(readme_setup):
    """Counter blocks 0xFE, 0xFF, 0x100 and their trivial ciphertexts."""
    _, iv, _ = readme_setup
    blocks = aes_128.counter_blocks(iv, CARRY_BLOCKS, first=CARRY_FIRST)
    cts = _trivial_blocks(blocks, BIG)
    return blocks, cts


def test_two_rounds_equal_per_block_path_and_oracle(gpu_context, oracle_keys, client, readme_setup, carry_case):
    key, iv, rk = readme_setup
    blocks, cts = carry_case
    assert aes_128.ctr_plan(iv, CARRY_FIRST, CARRY_BLOCKS) == 19
    out = E.ctr_keystream_raw(gpu_context, rk, iv, CARRY_FIRST, CARRY_BLOCKS, rounds=2)
    assert out.shape == (CARRY_BLOCKS, 128, BIG)
    assert np.array_equal(out, E.encrypt_blocks_raw(gpu_context, rk, cts, rounds=2))
    assert np.array_equal(out[2], oracle_keys.aes_encrypt_block(rk, cts[2], 2, threads=16))
    got = aes_128.bits_to_blocks(client.decrypt_bits_raw(out))
    assert got == aes_128.expand_key_and_encrypt_blocks(key, blocks, 2)


def test_one_round_dedup_feeds_final_kernel(gpu_context, client, readme_setup, carry_case):
    key, iv, rk = readme_setup
    blocks, cts = carry_case
    out = E.ctr_keystream_raw(gpu_context, rk, iv, CARRY_FIRST, CARRY_BLOCKS, rounds=1)
    assert np.array_equal(out, E.encrypt_blocks_raw(gpu_context, rk, cts, rounds=1))
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(out)) == aes_128.expand_key_and_encrypt_blocks(key, blocks, 1)


def test_ten_rounds_two_blocks(gpu_context, oracle_keys, client, readme_setup):
    key, iv, rk = readme_setup
    blocks = aes_128.counter_blocks(iv, 2)
    out = E.ctr_keystream_raw(gpu_context, rk, iv, 1, 2)
    got = aes_128.bits_to_blocks(client.decrypt_bits_raw(out))
    assert got == aes_128.expand_key_and_encrypt_blocks(key, blocks, 10)
    assert got[0].hex() == "175eea04466a73f066b5bc8195bf9e08"
    cts = _trivial_blocks(blocks, BIG)
    assert np.array_equal(out[0], oracle_keys.aes_encrypt_block(rk, cts[0], 10, threads=16))


def test_transcipher_37_bytes(gpu_context, client, readme_setup):
    """2 blocks + 5 bytes: only len*8 ciphertexts come back, each keystream bit + data bit << 63."""
    key, iv, rk = readme_setup
    msg = bytes((37 * i + 11) & 255 for i in range(37))
    data = aes_128.ctr_xor_plain(key, iv, 1, msg)  # what the client sends
    out = E.ctr_transcipher_raw(gpu_context, rk, iv, 1, data)
    assert out.shape == (37, 8, BIG)
    bits = client.decrypt_bits_raw(out).reshape(37, 8)
    assert bytes(aes_128.bits_to_u8(b) for b in bits) == aes_128.ctr_xor_plain(key, iv, 1, data) == msg
    ks = E.ctr_keystream_raw(gpu_context, rk, iv, 1, 3).reshape(48, 8, BIG)[:37]
    want = ks.copy()
    dbits = np.array([aes_128.u8_to_bits(d) for d in data], dtype=np.uint64)
    want[:, :, -1] += dbits << np.uint64(63)
    assert np.array_equal(out, want)
    assert E.ctr_transcipher_raw(gpu_context, rk, iv, 1, b"").shape == (0, 8, BIG)
    assert E.ctr_keystream_raw(gpu_context, rk, iv, 1, 0).shape == (0, 128, BIG)


def _check_one_round_transcipher(ctx, client, rk, key, iv, n_bytes, driver, lwe_size):
    """n_bytes from counter CARRY_FIRST with rounds=1: round 1 is the last, so the final kernel reads the SubBytes
    output through the plan's map, adds the data and stops at n_bytes.  Word for word the keystream's first n_bytes
    with the data bits << 63 on the body, and the plain one-round counter mode once decrypted."""
    nb = (n_bytes + 15) // 16
    msg = bytes((53 * i + 7) & 255 for i in range(n_bytes))
    blocks = aes_128.counter_blocks(iv, nb, first=CARRY_FIRST)
    ks_plain = b"".join(aes_128.expand_key_and_encrypt_blocks(key, blocks, 1))
    data = bytes(m ^ k for m, k in zip(msg, ks_plain))
    out = V.ctr_transcipher_raw(ctx, rk, iv, CARRY_FIRST, data, rounds=1)
    assert out.shape == (n_bytes, 8, lwe_size)
    want = driver.ctr_keystream_raw(ctx, rk, iv, CARRY_FIRST, nb, rounds=1).reshape(nb * 16, 8, lwe_size)[:n_bytes].copy()
    dbits = np.array([aes_128.u8_to_bits(d) for d in data], dtype=np.uint64)
    want[:, :, -1] += dbits << np.uint64(63)
    assert np.array_equal(out, want)
    bits = client.decrypt_bits_raw(out).reshape(n_bytes, 8)
    assert bytes(aes_128.bits_to_u8(b) for b in bits) == msg


def test_transcipher_one_round_21_bytes(gpu_context, client, readme_setup):
    """2 blocks, the second cut after 5 bytes."""
    key, iv, rk = readme_setup
    _check_one_round_transcipher(gpu_context, client, rk, key, iv, 21, E, BIG)


def test_transcipher_handles_noise_levels(gpu_context, client, readme_setup):
    """The handle variant on 5 bytes: the noise levels E.encrypt_blocks reports for 10 rounds on
    ctx.trivial inputs, and the raw entry point's words."""
    key, iv, rk = readme_setup
    ek = [gpu_context.bit_from_data(rk[i], 1) for i in range(44 * 32)]
    data = aes_128.ctr_xor_plain(key, iv, 1, b"hello")
    out = E.ctr_transcipher(gpu_context, ek, iv, 1, data)
    assert len(out) == 5 and all(len(byte) == 8 for byte in out)
    triv = [gpu_context.trivial(tfhe_aes.Cleartext(int(b))) for b in aes_128.blocks_to_bits(aes_128.counter_blocks(iv, 1))[0]]
    ref = E.encrypt_blocks(gpu_context, ek, triv, aes_128.ROUNDS)[0]
    assert [b.noise_level_squared for byte in out for b in byte] == \
        [b.noise_level_squared for byte in ref[:5] for b in byte]
    raw = E.ctr_transcipher_raw(gpu_context, rk, iv, 1, data)
    assert np.array_equal(np.stack([[b.data(BIG) for b in byte] for byte in out]), raw)
    assert aes_128.decrypt_byte_array(client, out) == b"hello"


def test_chunked_call_gives_the_same_words(gpu_context, product_raw, readme_setup, monkeypatch):
    """5 blocks in chunks of 2, 2, 1 (a plan per chunk) against one pass; the chunk size is read when the
    context is created."""
    _, iv, rk = readme_setup
    whole = E.ctr_keystream_raw(gpu_context, rk, iv, CARRY_FIRST, 5, rounds=1)
    monkeypatch.setenv("TAE_CTR_CHUNK_BLOCKS", "2")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_CTR_CHUNK_BLOCKS")
    assert np.array_equal(E.ctr_keystream_raw(ctx2, rk, iv, CARRY_FIRST, 5, rounds=1), whole)
    del ctx2


def test_device_memory(gpu_context, readme_setup):
    torch = pytest.importorskip("torch")
    _, iv, rk = readme_setup
    ref = E.ctr_keystream_raw(gpu_context, rk, iv, CARRY_FIRST, CARRY_BLOCKS, rounds=1)
    d_rk = torch.from_numpy(rk.view(np.int64)).to("cuda:0", non_blocking=True)
    d_out = torch.full((CARRY_BLOCKS, 128, BIG), -1, dtype=torch.int64, device="cuda:0")
    E.ctr_keystream_device(gpu_context, d_rk.data_ptr(), iv, CARRY_FIRST, CARRY_BLOCKS, 1, d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), ref)


def test_8bit_model(gpu_context8, oracle_keys8, product_raw8, readme_setup):
    key, iv, _ = readme_setup
    client8 = product_raw8[0]
    rk = client8.encrypt_bits_raw(_expanded_key_bits(key), start_index=310_000)
    blocks = aes_128.counter_blocks(iv, CARRY_BLOCKS, first=CARRY_FIRST)
    cts = _trivial_blocks(blocks, SMALL)
    out = A8.ctr_keystream_raw(gpu_context8, rk, iv, CARRY_FIRST, CARRY_BLOCKS, rounds=2)
    assert out.shape == (CARRY_BLOCKS, 128, SMALL)
    assert np.array_equal(out, A8.encrypt_blocks_raw(gpu_context8, rk, cts, rounds=2))
    got = aes_128.bits_to_blocks(client8.decrypt_bits_raw(out))
    assert got == aes_128.expand_key_and_encrypt_blocks(key, blocks, 2)
    one = A8.ctr_keystream_raw(gpu_context8, rk, iv, CARRY_FIRST, CARRY_BLOCKS, rounds=1)
    assert np.array_equal(one[0], oracle_keys8.aes8_encrypt_block(rk, cts[0], 1, threads=16))


def test_8bit_model_transcipher(gpu_context8, product_raw8, readme_setup):
    """The 8-bit model's transciphering with data: 5 bytes, one round."""
    key, iv, _ = readme_setup
    client8 = product_raw8[0]
    rk = client8.encrypt_bits_raw(_expanded_key_bits(key), start_index=310_000)
    _check_one_round_transcipher(gpu_context8, client8, rk, key, iv, 5, A8, SMALL)


def test_shortint_1bit_is_param_error(readme_setup):
    """The shortint_1bit set encodes bits differently (m << 62): refused before any device work."""
    _, iv, _ = readme_setup
    P5 = tfhe_aes.PARAMS_SHORTINT_1BIT
    _, keys = tfhe_aes.generate_keys_raw(P5, SEED, threads=16)
    ctx = tfhe_aes.context_from_raw(P5, keys, device=0)
    rk = np.zeros((44 * 32, ctx.lwe_size), dtype=np.uint64)
    for call in (lambda: E.ctr_keystream_raw(ctx, rk, iv, 1, 1),
                 lambda: E.ctr_transcipher_raw(ctx, rk, iv, 1, b"abc")):
        with pytest.raises(tfhe_aes.TaeError) as e:
            call()
        assert e.value.code == N.TAE_E_PARAM


def test_wrapping_range_is_arg_error(gpu_context, readme_setup):
    _, iv, rk = readme_setup
    with pytest.raises(tfhe_aes.TaeError) as e:
        E.ctr_keystream_raw(gpu_context, rk, iv, 2**64 - 1, 2, rounds=1)
    assert e.value.code == N.TAE_E_ARG
