"""Multi-key batches on the GPU (tae_aesm_*): key expansion, cipher, decryption keys, counter mode and CBC over a
key table, word for word against the single-key entry points (aes_var.GalMulAes) on each slot's key.

The circuit bootstrap is a pure function of its input ciphertext, so bits of different AES keys can share a launch
and every word of a batched call must equal the word the single-key call gives.  Full round counts are checked
through decryption.  ChaCha start indices from 8_000_000 up.
"""
import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_multi, aes_var

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
W = 32  # ciphertexts per word
V = aes_var.GalMulAes
M = aes_multi.GalMulAesMulti
K128 = [bytes(range(16)),                                  # FIPS-197 C.1
        bytes((7 * i + 3) & 255 for i in range(16)),
        bytes((29 * i + 101) & 255 for i in range(16))]
K256 = [bytes(range(32)), bytes((13 * i + 57) & 255 for i in range(32))]
FIPS_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
FIPS_CT_128 = bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a")
IV_A = bytes(range(0xC0, 0xC8))
IV16 = [bytes(range(0xA0, 0xB0)), bytes(range(0x50, 0x60))]


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _bytes_of(client, cts):
    bits = client.decrypt_bits_raw(cts).reshape(-1, 8)
    return bytes(aes_128.bits_to_u8(b) for b in bits)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def keys128(client):
    """Fresh encryptions of the three 128-bit keys, [3][128][BIG]."""
    return np.stack([client.encrypt_bits_raw(_bits(k), start_index=8_000_000 + 10_000 * i) for i, k in enumerate(K128)])


@pytest.fixture(scope="module")
def table128(gpu_context, keys128):
    """The three keys expanded by ONE batched call."""
    return M.key_schedule_raw(gpu_context, keys128)


@pytest.fixture(scope="module")
def single128(gpu_context, keys128):
    """The same keys expanded one by one by the single-key entry point: the yardstick."""
    return [V.key_schedule_raw(gpu_context, k) for k in keys128]


@pytest.fixture(scope="module")
def dtable128(gpu_context, table128):
    return M.decrypt_key_raw(gpu_context, table128)


@pytest.fixture(scope="module")
def table256(gpu_context, client):
    keys = np.stack([client.encrypt_bits_raw(_bits(k), start_index=8_100_000 + 10_000 * i) for i, k in enumerate(K256)])
    return keys, M.key_schedule_raw(gpu_context, keys)


# ---------------------------------------------------------------- 1. key expansion ----
def test_key_expansion_three_128_bit_keys(table128, single128, client):
    assert table128.shape == (3, 44 * W, BIG)
    for s in range(3):
        assert np.array_equal(table128[s], single128[s]), s  # all 1408 rows
    assert _bytes_of(client, table128[1]) == b"".join(aes_var.key_schedule_plain(K128[1]))


def test_key_expansion_two_256_bit_keys(gpu_context, client, table256):
    """Covers the SubWord-only step at i mod 8 = 4."""
    keys, table = table256
    assert table.shape == (2, 60 * W, BIG)
    for s in range(2):
        assert np.array_equal(table[s], V.key_schedule_raw(gpu_context, keys[s])), s
        assert _bytes_of(client, table[s]) == b"".join(aes_var.key_schedule_plain(K256[s]))


def test_key_expansion_nine_keys_runs_on_the_throughput_kernel(gpu_context, client, keys128, single128):
    """288 bits per identity bootstrap pass the latency kernel's 256: the step runs on br512x4."""
    plain = [K128[0], *(bytes((i * 17 + j * 5 + 1) & 255 for j in range(16)) for i in range(3)), K128[1],
             *(bytes((i * 31 + j * 11 + 9) & 255 for j in range(16)) for i in range(3)), K128[2]]
    keys = np.stack([client.encrypt_bits_raw(_bits(k), start_index=8_200_000 + 10_000 * i) for i, k in enumerate(plain)])
    for slot, i in ((0, 0), (4, 1), (8, 2)):
        keys[slot] = keys128[i]
    table = M.key_schedule_raw(gpu_context, keys)
    assert table.shape == (9, 44 * W, BIG)
    for slot, i in ((0, 0), (4, 1), (8, 2)):
        assert np.array_equal(table[slot], single128[i]), slot
    for s in range(9):
        assert _bytes_of(client, table[s]) == b"".join(aes_var.key_schedule_plain(plain[s])), s


def test_key_expansion_device_memory(gpu_context, keys128, table128):
    torch = pytest.importorskip("torch")
    d_keys = torch.from_numpy(keys128.view(np.int64)).to("cuda:0")
    d_table = torch.full((3, 44 * W, BIG), -1, dtype=torch.int64, device="cuda:0")
    M.key_schedule_device(gpu_context, 128, d_keys.data_ptr(), 3, d_table.data_ptr())
    assert np.array_equal(d_table.cpu().numpy().view(np.uint64), table128)


# ---------------------------------------------------------------- 2. cipher and inverse cipher ----
KEY_OF = [2, 0, 2, 1, 0]


def _pts():
    return [bytes((i * 53 + j * 19 + 7) & 255 for j in range(16)) for i in range(5)]


def test_encrypt_blocks_per_slot(gpu_context, client, table128):
    pts = _pts()
    blocks = client.encrypt_bits_raw(aes_128.blocks_to_bits(pts).reshape(-1), start_index=8_300_000).reshape(5, 128, BIG)
    for r in (1, 2):
        out = M.encrypt_blocks_raw(gpu_context, table128, KEY_OF, blocks, r)
        assert out.shape == (5, 128, BIG)
        for i, k in enumerate(KEY_OF):
            assert np.array_equal(out[i:i + 1], V.encrypt_blocks_raw(gpu_context, table128[k], blocks[i:i + 1], r)), (r, i)
    want = [aes_var.encrypt_block_plain(aes_var.key_schedule_plain(K128[k]), p, 2) for k, p in zip(KEY_OF, pts)]
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(out)) == want
    assert M.encrypt_blocks_raw(gpu_context, table128, [], blocks[:0], 1).shape == (0, 128, BIG)


def test_decrypt_blocks_per_slot(gpu_context, client, dtable128):
    pts = _pts()
    cts2 = [aes_var.encrypt_block_plain(aes_var.key_schedule_plain(K128[k]), p, 2) for k, p in zip(KEY_OF, pts)]
    blocks = client.encrypt_bits_raw(aes_128.blocks_to_bits(cts2).reshape(-1), start_index=8_310_000).reshape(5, 128, BIG)
    for r in (1, 2):
        out = M.decrypt_blocks_raw(gpu_context, dtable128, KEY_OF, blocks, r)
        for i, k in enumerate(KEY_OF):
            assert np.array_equal(out[i:i + 1], V.decrypt_blocks_raw(gpu_context, dtable128[k], blocks[i:i + 1], r)), (r, i)
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(out)) == pts


def test_unreferenced_slot_is_not_read(gpu_context, client, table128):
    """A stale slot (here: garbage) changes nothing for blocks that do not name it."""
    blocks = client.encrypt_bits_raw(aes_128.blocks_to_bits(_pts()[:2]).reshape(-1), start_index=8_320_000).reshape(2, 128, BIG)
    stale = table128.copy()
    stale[1] = np.uint64(0xDEADBEEF)
    assert np.array_equal(M.encrypt_blocks_raw(gpu_context, stale, [2, 0], blocks, 1),
                          M.encrypt_blocks_raw(gpu_context, table128, [2, 0], blocks, 1))


# ---------------------------------------------------------------- 3. decryption keys ----
def test_decrypt_keys_two_256_bit_slots(gpu_context, client, table256):
    _, table = table256
    dtable = M.decrypt_key_raw(gpu_context, table)
    assert dtable.shape == table.shape
    for s in range(2):
        assert np.array_equal(dtable[s], V.decrypt_key_raw(gpu_context, table[s])), s
    assert _bytes_of(client, dtable[1]) == b"".join(aes_var.decrypt_key_plain(aes_var.key_schedule_plain(K256[1])))


def test_decrypt_keys_128_equal_single(gpu_context, table128, dtable128):
    assert np.array_equal(dtable128[2], V.decrypt_key_raw(gpu_context, table128[2]))


# ---------------------------------------------------------------- 4. counter mode ----
MSG = [bytes((41 * i + 3) & 255 for i in range(37)), bytes((17 * i + 88) & 255 for i in range(32)), b"hello"]
CTR = [(0, IV_A, 255), (1, IV_A, 255), (0, IV_A, 256)]  # slot, iv, first counter


def _ctr_streams():
    """Stream 0 carries into byte 14 and has a partial last block, stream 1 has the same public bytes under
    another key, stream 2 shares groups with stream 0."""
    return [(slot, iv, first, aes_var.ctr_xor_plain(K128[slot], iv, first, msg)) for (slot, iv, first), msg in zip(CTR, MSG)]


@pytest.fixture(scope="module")
def ctr_out(gpu_context, table128):
    streams = _ctr_streams()
    return {r: M.ctr_transcipher_raw(gpu_context, table128, streams, r) for r in (1, 2)}


@pytest.mark.parametrize("r", [1, 2])
def test_ctr_streams_equal_single_key_calls(gpu_context, client, table128, ctr_out, r):
    streams = _ctr_streams()
    assert [o.shape for o in ctr_out[r]] == [(37, 8, BIG), (32, 8, BIG), (5, 8, BIG)]
    for (slot, iv, first, data), got in zip(streams, ctr_out[r]):
        assert np.array_equal(got, V.ctr_transcipher_raw(gpu_context, table128[slot], iv, first, data, rounds=r))


def test_ctr_plan_count(gpu_context):
    streams = _ctr_streams()
    want = set()
    for slot, iv, first, data in streams:
        for blk in aes_128.counter_blocks(iv, (len(data) + 15) // 16, first=first):
            want |= {(slot, pos, blk[pos]) for pos in range(16)}
    # slot 0: counters 255..257 (8 iv + 6 constant bytes + 2 values of byte 14 + 3 of byte 15); slot 1: 255, 256
    assert M.ctr_plan(streams) == len(want) == 19 + 18


def test_ctr_chunked_call_gives_the_same_words(product_raw, table128, ctr_out, monkeypatch):
    """6 blocks in chunks of 2: the boundaries fall inside stream 0 and between streams."""
    monkeypatch.setenv("TAE_CTR_CHUNK_BLOCKS", "2")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_CTR_CHUNK_BLOCKS")
    for r in (1, 2):
        got = M.ctr_transcipher_raw(ctx2, table128, _ctr_streams(), r)
        for a, b in zip(got, ctr_out[r]):
            assert np.array_equal(a, b), r
    del ctx2


def test_ctr_keystream_without_data(gpu_context, table128):
    streams = [(slot, iv, first, None, len(msg)) for (slot, iv, first), msg in zip(CTR, MSG)]
    got = M.ctr_transcipher_raw(gpu_context, table128, streams, 2)
    for (slot, iv, first, _, n), ks in zip(streams, got):
        want = V.ctr_keystream_raw(gpu_context, table128[slot], iv, first, (n + 15) // 16, rounds=2)
        assert np.array_equal(ks, want.reshape(-1, 8, BIG)[:n])
    # a stream with data next to one without: zeros are XORed into the latter
    mixed = M.ctr_transcipher_raw(gpu_context, table128, [streams[2], _ctr_streams()[1]], 1)
    assert np.array_equal(mixed[0], V.ctr_keystream_raw(gpu_context, table128[0], IV_A, 256, 1, rounds=1).reshape(-1, 8, BIG)[:5])
    assert M.ctr_transcipher_raw(gpu_context, table128, [], 1) == []
    assert [o.shape for o in M.ctr_transcipher_raw(gpu_context, table128, [(0, IV_A, 1, b"")], 1)] == [(0, 8, BIG)]


def test_ctr_device_memory(gpu_context, table128, ctr_out):
    torch = pytest.importorskip("torch")
    d_table = torch.from_numpy(table128.view(np.int64)).to("cuda:0")
    d_out = torch.full((74, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    M.ctr_transcipher_device(gpu_context, 128, d_table.data_ptr(), 3, _ctr_streams(), 1, d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), np.concatenate(ctr_out[1]))


# ---------------------------------------------------------------- 5. CBC ----
def test_cbc_two_streams(gpu_context, client, dtable128):
    msgs = [bytes((37 * i + 11) & 255 for i in range(32)), bytes((3 * i + 200) & 255 for i in range(16))]
    slots = [2, 0]
    streams = [(s, iv, aes_var.cbc_encrypt_plain(K128[s], iv, m)) for s, iv, m in zip(slots, IV16, msgs)]
    out = M.cbc_transcipher_raw(gpu_context, dtable128, streams, 2)
    assert [o.shape for o in out] == [(32, 8, BIG), (16, 8, BIG)]
    for (s, iv, data), got in zip(streams, out):
        assert np.array_equal(got, V.cbc_transcipher_raw(gpu_context, dtable128[s], iv, data, rounds=2))


# ---------------------------------------------------------------- 6. full rounds ----
def test_full_rounds_ctr_and_handles(gpu_context, client, keys128, table128):
    msgs = [FIPS_PT, bytes((91 * i + 5) & 255 for i in range(16))]
    streams = [(s, IV_A, 1 + s, aes_var.ctr_xor_plain(K128[s], IV_A, 1 + s, m)) for s, m in enumerate(msgs)]
    out = M.ctr_transcipher_raw(gpu_context, table128[:2], streams)  # 10 rounds
    assert [_bytes_of(client, o) for o in out] == msgs
    # the C.1 key really is slot 0: one block through the 10-round cipher
    blk = client.encrypt_bits_raw(aes_128.blocks_to_bits([FIPS_PT]).reshape(-1), start_index=8_400_000).reshape(1, 128, BIG)
    enc = M.encrypt_blocks_raw(gpu_context, table128, [0], blk)
    assert aes_128.bits_to_blocks(client.decrypt_bits_raw(enc)) == [FIPS_CT_128]
    # handles: the table at noise level 1, the outputs at 9
    hkeys = [[gpu_context.bit_from_data(keys128[s][i], 1) for i in range(128)] for s in range(2)]
    table = M.key_schedule(gpu_context, hkeys)
    assert len(table) == 2 and all(len(k) == 44 for k in table)
    flat = [[b for w in k for byte in w for b in byte] for k in table]
    assert {b.noise_level_squared for k in flat for b in k} == {1}
    for s in range(2):
        for i in (0, 127, 128, 44 * W - 1):
            assert np.array_equal(flat[s][i].data(BIG), table128[s][i])
    got = M.ctr_transcipher(gpu_context, [table[0], None, table[1]], [(2, IV_A, 2, streams[1][3]), (0, IV_A, 1, streams[0][3])])
    assert [len(g) for g in got] == [16, 16]
    assert {b.noise_level_squared for g in got for byte in g for b in byte} == {9}
    assert [aes_128.decrypt_byte_array(client, g) for g in got] == [msgs[1], msgs[0]]


def test_cbc_handles(gpu_context, client, dtable128):
    msg = bytes((5 * i + 1) & 255 for i in range(16))
    data = aes_var.cbc_encrypt_plain(K128[1], IV16[0], msg)
    dk = [gpu_context.bit_from_data(dtable128[1][i], 1) for i in range(44 * W)]
    got = M.cbc_transcipher(gpu_context, [None, dk], [(1, IV16[0], data)])
    assert {b.noise_level_squared for byte in got[0] for b in byte} == {9}
    assert aes_128.decrypt_byte_array(client, got[0]) == msg


# ---------------------------------------------------------------- 7. errors ----
def test_argument_errors(gpu_context, table128):
    blocks = np.zeros((1, 128, BIG), dtype=np.uint64)
    for bad in (-1, 3):
        assert _code(lambda: M.encrypt_blocks_raw(gpu_context, table128, [bad], blocks, 1)) == N.TAE_E_ARG
        assert _code(lambda: M.decrypt_blocks_raw(gpu_context, table128, [bad], blocks, 1)) == N.TAE_E_ARG
        assert _code(lambda: M.ctr_transcipher_raw(gpu_context, table128, [(bad, IV_A, 1, b"abc")], 1)) == N.TAE_E_ARG
        assert _code(lambda: M.cbc_transcipher_raw(gpu_context, table128, [(bad, IV16[0], bytes(16))], 1)) == N.TAE_E_ARG
    assert _code(lambda: M.encrypt_blocks_raw(gpu_context, table128[:0], [0], blocks, 1)) == N.TAE_E_ARG  # no keys
    assert _code(lambda: M.encrypt_blocks_raw(gpu_context, table128[:, :-1], [0], blocks, 1)) == N.TAE_E_ARG
    assert _code(lambda: M.ctr_transcipher_raw(gpu_context, table128[:, :-W], [(0, IV_A, 1, b"abc")], 1)) == N.TAE_E_ARG
    assert _code(lambda: M.ctr_transcipher_raw(gpu_context, table128, [(0, IV_A, 2**64 - 1, bytes(17))], 1)) == N.TAE_E_ARG
    assert _code(lambda: M.cbc_transcipher_raw(gpu_context, table128, [(0, IV16[0], bytes(17))], 1)) == N.TAE_E_ARG
    for call in (lambda: M.encrypt_blocks_raw(gpu_context, table128, [0], blocks, 11),
                 lambda: M.decrypt_blocks_raw(gpu_context, table128, [0], blocks, 11),
                 lambda: M.ctr_transcipher_raw(gpu_context, table128, [(0, IV_A, 1, b"abc")], 11),
                 lambda: M.cbc_transcipher_raw(gpu_context, table128, [(0, IV16[0], bytes(16))], 0)):
        assert _code(call) == N.TAE_E_PARAM
    lib = tfhe_aes.lib()  # a key size that no array has
    ko = np.zeros(1, dtype=np.int32)
    assert lib.tae_aesm_encrypt_blocks_raw(gpu_context._h, 160, table128.ctypes.data, 3, ko.ctypes.data, blocks.ctypes.data,
                                           1, 1, blocks.ctypes.data, N.TAE_MEM_HOST) == N.TAE_E_PARAM
    # nothing to do is TAE_OK
    assert M.key_schedule_raw(gpu_context, np.zeros((0, 128, BIG), dtype=np.uint64)).shape == (0, 44 * W, BIG)
    assert M.decrypt_key_raw(gpu_context, table128[:0]).shape == (0, 44 * W, BIG)


def test_8bit_model_is_param_error(gpu_context8):
    L = gpu_context8.lwe_size
    blocks = np.zeros((1, 128, L), dtype=np.uint64)
    table = np.zeros((2, 44 * W, L), dtype=np.uint64)
    keys = np.zeros((2, 128, L), dtype=np.uint64)
    bit = gpu_context8.trivial(tfhe_aes.Cleartext(0))
    for call in (lambda: M.key_schedule_raw(gpu_context8, keys),
                 lambda: M.decrypt_key_raw(gpu_context8, table),
                 lambda: M.encrypt_blocks_raw(gpu_context8, table, [1], blocks, 1),
                 lambda: M.decrypt_blocks_raw(gpu_context8, table, [1], blocks, 1),
                 lambda: M.ctr_transcipher_raw(gpu_context8, table, [(0, IV_A, 1, b"abc")], 1),
                 lambda: M.cbc_transcipher_raw(gpu_context8, table, [(0, IV16[0], bytes(16))], 1),
                 lambda: M.key_schedule(gpu_context8, [[bit] * 128]),
                 lambda: M.ctr_transcipher(gpu_context8, [[bit] * (44 * W)], [(0, IV_A, 1, b"abc")], 1),
                 lambda: M.cbc_transcipher(gpu_context8, [[bit] * (44 * W)], [(0, IV16[0], bytes(16))], 1)):
        assert _code(call) == N.TAE_E_PARAM
