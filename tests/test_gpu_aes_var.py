"""AES-192 and AES-256 on the GPU (tae_aesx_*; FIPS-197 5.2 and figure 11, the reference is AES-128 only): the
key expansion on the device, and the cipher, counter mode, inverse cipher and CBC with 52- and 60-word keys.

Word-for-word anchors.  The circuit bootstrap is deterministic in its input ciphertexts, so
- the device key expansion at 128 bits must equal the host-driven key schedule of aes_128,
- single expansion steps at 192 and 256 bits must equal the CPU oracle's circuit_bootstrap around numpy
  uint64 additions, computed on the product's own earlier words,
- a run of R <= 2 rounds reads round keys 0, 1 and Nr only, so a 60- (52-) word key must give what the
  128-bit entry points give on its words 0..39 and 56..59 (48..51).
Full round counts are checked through decryption against the FIPS-197 C.2 and C.3 vectors.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
E = aes_128.ShortintWoppbs1BitSboxGalMulPbsAesEncrypt
V = aes_var.GalMulAes
KEYS = {128: bytes(range(16)), 192: bytes(range(24)), 256: bytes(range(32))}
FIPS_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
FIPS_CT = {192: bytes.fromhex("dda97ca4864cdfe06eaf70a0ec0d7191"),   # FIPS-197 C.2
           256: bytes.fromhex("8ea2b7ca516745bfeafc49904b496089")}   # FIPS-197 C.3
IV8 = bytes(range(0xC0, 0xC8))
IV16 = bytes(range(0xA0, 0xB0))
W = 32  # ciphertexts per word


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _bytes_of(client, cts):
    bits = client.decrypt_bits_raw(cts).reshape(-1, 8)
    return bytes(aes_128.bits_to_u8(b) for b in bits)


def _trivial_blocks(blocks):
    bits = aes_128.blocks_to_bits(blocks).astype(np.uint64)
    cts = np.zeros((len(blocks), 128, BIG), dtype=np.uint64)
    cts[:, :, -1] = bits << np.uint64(63)
    return cts


def _fold44(key):
    """Words 0..39 and the last four of a 52- or 60-word key: what R <= 10 rounds of the 128-bit paths read
    where the same R rounds of the longer key read 0..4R-1 and 4Nr..4Nr+3."""
    return np.concatenate([key[:40 * W], key[-4 * W:]])


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def rk_dev(gpu_context, client):
    """Expanded keys made on the device from fresh encryptions of KEYS[192] and KEYS[256]."""
    out = {}
    for i, kb in enumerate((192, 256)):
        key = client.encrypt_bits_raw(_bits(KEYS[kb]), start_index=6_000_000 + 1000 * i)
        out[kb] = (key, V.key_schedule_raw(gpu_context, key))
    return out


@pytest.fixture(scope="module")
def rk_fresh(client):
    """Fresh encryptions of the PLAIN expanded keys [W*32][BIG]: inputs of the word-for-word comparisons."""
    return {kb: client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(KEYS[kb]))),
                                        start_index=6_010_000 + 10_000 * i)
            for i, kb in enumerate((192, 256))}


@pytest.fixture(scope="module")
def dk256(gpu_context, rk_fresh):
    return V.decrypt_key_raw(gpu_context, rk_fresh[256])


@pytest.fixture(scope="module")
def luts(oracle_mod, oracle_keys):
    n = oracle_keys.p["N"]
    return {"sbox": oracle_mod.generate_lut(n, 8, 8, lambda x: aes_128.SBOX[x]),
            "id1": oracle_mod.generate_lut(n, 1, 1, lambda x: x)}


def _cbs_many(oracle_keys, groups, lut, n_out):
    with ThreadPoolExecutor(max_workers=16) as pool:
        return np.stack(list(pool.map(lambda g: oracle_keys.circuit_bootstrap(g, lut, n_out), groups)))


def _oracle_word(oracle_keys, luts, rk, nk, i):
    """Word i of the expansion from the product's words i - nk and i - 1: the step of FIPS-197 figure 11 as
    uint64 additions of whole ciphertexts, then the identity bootstrap of its 32 bits."""
    back = rk[(i - nk) * W:(i - nk + 1) * W]
    prev = rk[(i - 1) * W:i * W]
    if i % nk == 0 or (nk == 8 and i % 8 == 4):
        sub = _cbs_many(oracle_keys, prev.reshape(4, 8, BIG), luts["sbox"], 8)  # SubWord, byte by byte
        if i % nk == 0:
            sub = np.roll(sub, -1, axis=0)  # RotWord: byte b takes the S-box of byte b + 1
        t = back + sub.reshape(W, BIG)
        if i % nk == 0:
            rcon = np.array(aes_128.u8_to_bits(aes_128.RC[i // nk]), dtype=np.uint64)
            t[:8, -1] += rcon << np.uint64(63)
    else:
        t = back + prev
    return _cbs_many(oracle_keys, t.reshape(W, 1, BIG), luts["id1"], 1).reshape(W, BIG)


# ---------------------------------------------------------------- 1. key expansion at 128 bits ----
def test_key_expansion_128_equals_host_driven_schedule(gpu_context, client):
    key = client.encrypt_bits_raw(_bits(KEYS[128]), start_index=6_005_000)
    got = V.key_schedule_raw(gpu_context, key)
    want = E.key_schedule_raw(gpu_context, key)
    assert got.shape == want.shape == (44 * W, BIG)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 2. key expansion at 192 / 256 bits ----
@pytest.mark.parametrize("kb, words", [(256, (8, 12, 13)), (192, (6, 7))])
def test_key_expansion_steps_equal_oracle(gpu_context, oracle_keys, client, rk_dev, luts, kb, words):
    """256: word 8 = RotWord + SubWord + Rcon, word 12 = SubWord alone, word 13 = plain XOR; 192: words 6, 7."""
    key, rk = rk_dev[kb]
    nk = kb // 32
    assert rk.shape == ((4 * (nk + 7)) * W, BIG)
    assert np.array_equal(rk[:kb], key)
    for i in words:
        assert np.array_equal(rk[i * W:(i + 1) * W], _oracle_word(oracle_keys, luts, rk, nk, i)), i
    assert _bytes_of(client, rk) == b"".join(aes_var.key_schedule_plain(KEYS[kb]))


def test_key_expansion_device_memory_and_handles(gpu_context, client, rk_dev):
    """The device-pointer entry gives the host entry's words; the handle entry the bookkeeping of the replay."""
    torch = pytest.importorskip("torch")
    key, rk = rk_dev[192]
    d_key = torch.from_numpy(key.view(np.int64)).to("cuda:0")
    d_rk = torch.full((52 * W, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.key_schedule_device(gpu_context, 192, d_key.data_ptr(), d_rk.data_ptr())
    assert np.array_equal(d_rk.cpu().numpy().view(np.uint64), rk)
    ek = V.key_schedule(gpu_context, [gpu_context.bit_from_data(key[i], 1) for i in range(192)])
    flat = [b for w in ek for byte in w for b in byte]
    assert len(ek) == 52 and {b.noise_level_squared for b in flat} == {1}
    for i in (0, 191, 192, 52 * W - 1):
        assert np.array_equal(flat[i].data(BIG), rk[i])


# ---------------------------------------------------------------- 3. cipher offsets ----
@pytest.mark.parametrize("kb", [256, 192])
def test_short_runs_equal_128_bit_path_on_folded_key(gpu_context, oracle_keys, client, rk_fresh, golden, kb):
    rk = rk_fresh[kb]
    rk44 = _fold44(rk)
    pts = [bytes.fromhex(golden["chacha20_zero_seed"][b]) for b in ("block1", "block2")]
    blocks = client.encrypt_bits_raw(aes_128.blocks_to_bits(pts).reshape(-1), start_index=6_040_000 + kb)
    blocks = blocks.reshape(2, 128, BIG)
    ek = aes_var.key_schedule_plain(KEYS[kb])
    for r in (1, 2):
        out = V.encrypt_blocks_raw(gpu_context, rk, blocks, r)
        assert np.array_equal(out, E.encrypt_blocks_raw(gpu_context, rk44, blocks, r)), r
        assert aes_128.bits_to_blocks(client.decrypt_bits_raw(out)) == [aes_var.encrypt_block_plain(ek, p, r) for p in pts]
    if kb == 256:
        assert np.array_equal(out[1], oracle_keys.aes_encrypt_block(rk44, blocks[1], 2, threads=16))


# ---------------------------------------------------------------- 4. full rounds ----
@pytest.mark.parametrize("kb", [256, 192])
def test_fips197_vector_with_device_expanded_key(gpu_context, client, rk_dev, kb):
    block = client.encrypt_bits_raw(aes_128.blocks_to_bits([FIPS_PT]).reshape(-1), start_index=6_050_000 + kb)
    out = V.encrypt_blocks_raw(gpu_context, rk_dev[kb][1], block.reshape(1, 128, BIG))
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(out)) == [FIPS_CT[kb]]


# ---------------------------------------------------------------- 5. counter mode ----
def test_ctr_256(gpu_context, client, rk_fresh):
    rk = rk_fresh[256]
    ks = V.ctr_keystream_raw(gpu_context, rk, IV8, 255, 3, rounds=2)  # counters 255, 256, 257: a carry into byte 14
    want = V.encrypt_blocks_raw(gpu_context, rk, _trivial_blocks(aes_128.counter_blocks(IV8, 3, first=255)), 2)
    assert ks.shape == (3, 128, BIG) and np.array_equal(ks, want)
    msg = bytes((41 * i + 3) & 255 for i in range(37))
    data = aes_var.ctr_xor_plain(KEYS[256], IV8, 255, msg)
    out = V.ctr_transcipher(gpu_context, [gpu_context.bit_from_data(rk[i], 1) for i in range(60 * W)], IV8, 255, data)
    assert len(out) == 37 and {b.noise_level_squared for byte in out for b in byte} == {9}
    assert aes_128.decrypt_byte_array(client, out) == msg


# ---------------------------------------------------------------- 6. inverse cipher ----
def test_decrypt_key_256(gpu_context, client, rk_fresh, dk256):
    rk = rk_fresh[256]
    assert dk256.shape == (60 * W, BIG)
    assert np.array_equal(dk256[:4 * W], rk[:4 * W]) and np.array_equal(dk256[56 * W:], rk[56 * W:])
    dk44 = E.decrypt_key_raw(gpu_context, _fold44(rk))
    assert np.array_equal(dk256[4 * W:40 * W], dk44[4 * W:40 * W])
    assert _bytes_of(client, dk256) == b"".join(aes_var.decrypt_key_plain(aes_var.key_schedule_plain(KEYS[256])))


def test_decrypt_blocks_256(gpu_context, client, rk_fresh, dk256, golden):
    ek = aes_var.key_schedule_plain(KEYS[256])
    pts = [FIPS_PT, bytes.fromhex(golden["chacha20_zero_seed"]["block2"])]
    cts2 = [aes_var.encrypt_block_plain(ek, p, 2) for p in pts]
    blocks = client.encrypt_bits_raw(aes_128.blocks_to_bits(cts2).reshape(-1), start_index=6_060_000).reshape(2, 128, BIG)
    out = V.decrypt_blocks_raw(gpu_context, dk256, blocks, 2)
    assert np.array_equal(out, E.decrypt_blocks_raw(gpu_context, _fold44(dk256), blocks, 2))
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(out)) == pts
    # 14 rounds: the raw round trip
    x = client.encrypt_bits_raw(aes_128.blocks_to_bits(pts).reshape(-1), start_index=6_061_000).reshape(2, 128, BIG)
    enc = V.encrypt_blocks_raw(gpu_context, rk_fresh[256], x)
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(enc)) == [FIPS_CT[256], aes_var.encrypt_block_plain(ek, pts[1])]
    back = V.decrypt_blocks_raw(gpu_context, dk256, enc)
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(back)) == pts


def test_handles_round_trip_256_is_not_independent(gpu_context, client, rk_fresh):
    """encrypt_blocks' output carries the ids of round key 14, which the decryption key keeps at words 56..59."""
    rk = rk_fresh[256]
    ek = [gpu_context.bit_from_data(rk[i], 1) for i in range(60 * W)]
    dk = V.decrypt_key(gpu_context, ek)
    flat = [b for w in dk for byte in w for b in byte]
    assert len(dk) == 60 and {b.noise_level_squared for b in flat[4 * W:56 * W]} == {1}
    assert np.array_equal(flat[57 * W].data(BIG), rk[57 * W])
    enc = V.encrypt_block_for_rounds(gpu_context, ek, aes_128.encrypt_byte_array(client, FIPS_PT), 1)
    with pytest.raises(tfhe_aes.NoiseNotIndependent):
        V.decrypt_block_for_rounds(gpu_context, dk, enc, 1)
    ct = aes_var.encrypt_block_plain(aes_var.key_schedule_plain(KEYS[256]), FIPS_PT, 1)
    assert aes_128.decrypt_byte_array(client, enc) == ct
    out = V.decrypt_block_for_rounds(gpu_context, dk, aes_128.encrypt_byte_array(client, ct), 1)
    assert {b.noise_level_squared for byte in out for b in byte} == {9}
    assert aes_128.decrypt_byte_array(client, out) == FIPS_PT


# ---------------------------------------------------------------- 7. CBC ----
def test_cbc_256(gpu_context, client, dk256):
    msg = bytes((37 * i + 11) & 255 for i in range(43))
    padded = msg + bytes([5] * 5)  # PKCS#7 to 48 bytes: the client's business
    data = aes_var.cbc_encrypt_plain(KEYS[256], IV16, padded)
    out = V.cbc_transcipher_raw(gpu_context, dk256, IV16, data)
    assert out.shape == (48, 8, BIG)
    assert _bytes_of(client, out) == aes_var.cbc_decrypt_plain(KEYS[256], IV16, data) == padded
    # two rounds: the 128-bit paths on the folded key, the mode itself and the block call it is made of
    dk44 = _fold44(dk256)
    out2 = V.cbc_transcipher_raw(gpu_context, dk256, IV16, data, rounds=2)
    assert np.array_equal(out2, V.cbc_transcipher_raw(gpu_context, dk44, IV16, data, rounds=2))
    blocks = [data[i:i + 16] for i in (0, 16, 32)]
    want = E.decrypt_blocks_raw(gpu_context, dk44, _trivial_blocks(blocks), 2).reshape(48, 8, BIG)
    prev = np.array([aes_128.u8_to_bits(b) for b in IV16 + data[:32]], dtype=np.uint64)
    want[:, :, -1] += prev << np.uint64(63)
    assert np.array_equal(out2, want)


# ---------------------------------------------------------------- 8. errors ----
def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def test_argument_errors(gpu_context):
    blocks = np.zeros((1, 128, BIG), dtype=np.uint64)
    k44, k52, k60 = (np.zeros((w * W, BIG), dtype=np.uint64) for w in (44, 52, 60))
    assert _code(lambda: V.encrypt_blocks_raw(gpu_context, k52, blocks, 1, key_bits=256)) == N.TAE_E_ARG
    assert _code(lambda: V.decrypt_blocks_raw(gpu_context, k52, blocks, 1, key_bits=256)) == N.TAE_E_ARG
    assert _code(lambda: V.encrypt_blocks_raw(gpu_context, k52[:-W], blocks, 1)) == N.TAE_E_ARG
    triv = [gpu_context.trivial(tfhe_aes.Cleartext(0))] * (52 * W)
    assert _code(lambda: V.encrypt_blocks(gpu_context, triv, [], 1, key_bits=256)) == N.TAE_E_ARG
    assert _code(lambda: V.encrypt_blocks_raw(gpu_context, k60, blocks, 15)) == N.TAE_E_PARAM
    assert _code(lambda: V.encrypt_blocks_raw(gpu_context, k44, blocks, 11)) == N.TAE_E_PARAM
    assert _code(lambda: V.decrypt_blocks_raw(gpu_context, k60, blocks, 15)) == N.TAE_E_PARAM
    assert _code(lambda: V.ctr_keystream_raw(gpu_context, k52, IV8, 1, 1, rounds=13)) == N.TAE_E_PARAM
    assert _code(lambda: V.cbc_transcipher_raw(gpu_context, k60, IV16, bytes(16), rounds=0)) == N.TAE_E_PARAM
    assert _code(lambda: V.cbc_transcipher_raw(gpu_context, k60, IV16, bytes(17))) == N.TAE_E_ARG
    lib = tfhe_aes.lib()  # a key size that no array has
    assert lib.tae_aesx_encrypt_blocks_raw(gpu_context._h, 160, k60.ctypes.data, blocks.ctypes.data, 1, 1,
                                           blocks.ctypes.data, N.TAE_MEM_HOST) == N.TAE_E_PARAM


def test_8bit_model_is_param_error(gpu_context8):
    L = gpu_context8.lwe_size
    blocks = np.zeros((1, 128, L), dtype=np.uint64)
    for w in (52, 60):
        key = np.zeros((w * W, L), dtype=np.uint64)
        for call in (lambda: V.encrypt_blocks_raw(gpu_context8, key, blocks, 1),
                     lambda: V.ctr_keystream_raw(gpu_context8, key, IV8, 1, 1),
                     lambda: V.decrypt_key_raw(gpu_context8, key),
                     lambda: V.decrypt_blocks_raw(gpu_context8, key, blocks, 1),
                     lambda: V.cbc_transcipher_raw(gpu_context8, key, IV16, bytes(16)),
                     lambda: V.key_schedule_raw(gpu_context8, key[:(w - 28) * 8])):
            assert _code(call) == N.TAE_E_PARAM
