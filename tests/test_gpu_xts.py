"""XTS-AES decryption of a public ciphertext on the GPU (tae_aesx_xts_*, tae_stage_xts_masks; IEEE 1619,
DESIGN.md 5.12; the reference has no XTS).

Word-for-word anchors.  The pipeline is deterministic in its input ciphertexts, so
- the tweak call must equal the existing block cipher on trivial encryptions of the tweaks followed by the existing
  1 -> 1 identity circuit bootstrap,
- the mask stage must equal numpy uint64 sums of the tweak ciphertexts chosen by this file's own restatement of the
  byte-wise alpha step of IEEE 1619 (`_alpha`, `_mask_rows`: no table of the product is read),
- the transcipher call must equal the existing inverse cipher on trivial(C) + masks, plus the masks.
Full round counts are checked through decryption against an IEEE 1619 vector and the plain model.
"""
import functools

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
V = aes_var.GalMulAes
W = 32
# IEEE 1619 vector 2
KEY1, KEY2, UNIT = bytes([0x11] * 16), bytes([0x22] * 16), 0x3333333333
PT = bytes([0x44] * 32)
CT = bytes.fromhex("c454185e6a16936e39334038acef838bfb186fff7480adc4289382ecd6d394f0")
INDICES = (0, 1, 2, 7, 8, 121, 122, 127, 128, 255, 4095)


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


def _alpha(t):
    """IEEE 1619 5.2 on rows of 16 bytes [n][16]: every byte shifted left by one with the carry of the byte before
    it, 0x87 into byte 0 on carry out of byte 15."""
    out = (t << 1) & 0xFF
    out[:, 1:] |= t[:, :-1] >> 7
    out[:, 0] ^= 0x87 * (t[:, 15] >> 7)
    return out


@functools.lru_cache(maxsize=None)
def _mask_rows(j):
    """Row o (MSB-first ciphertext index) of alpha^j: the source ciphertexts, from the images of the 128 unit
    vectors under j byte-wise steps."""
    t = np.zeros((128, 16), dtype=np.uint16)
    for src in range(128):
        t[src, src >> 3] = 0x80 >> (src & 7)
    for _ in range(j):
        t = _alpha(t)
    bits = np.unpackbits(t.astype(np.uint8), axis=1)  # [src][o], MSB first
    return [[int(s) for s in np.nonzero(bits[:, o])[0]] for o in range(128)]


def _masks_np(tweaks_ct, unit_of, index):
    out = np.zeros((len(index), 128, BIG), dtype=np.uint64)
    for b, (u, j) in enumerate(zip(unit_of, index)):
        for o, srcs in enumerate(_mask_rows(j)):
            out[b, o] = tweaks_ct[u, srcs].sum(axis=0, dtype=np.uint64)
    return out


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def keys128(gpu_context, client):
    """Fresh encryptions of the plain expanded keys of vector 2, and the decryption key of key 1."""
    rk1 = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(KEY1))), start_index=7_000_000)
    rk2 = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(KEY2))), start_index=7_010_000)
    return V.decrypt_key_raw(gpu_context, rk1), rk2


@pytest.fixture(scope="module")
def tweaks2(gpu_context, keys128):
    """Real tweak ciphertexts of two data units (two rounds)."""
    return V.xts_tweaks_raw(gpu_context, keys128[1], [UNIT, 7], rounds=2)


def test_tweaks_equal_composition(gpu_context, client, keys128):
    _, rk2 = keys128
    tweaks = [UNIT, 9, UNIT]
    got = V.xts_tweaks_raw(gpu_context, rk2, tweaks, rounds=2)
    assert got.shape == (3, 128, BIG)
    blocks = [t.to_bytes(16, "little") for t in tweaks]
    enc = V.encrypt_blocks_raw(gpu_context, rk2, _trivial_blocks(blocks), 2)
    ident = gpu_context.generate_lookup_table(1, 1, lambda x: x)
    want = gpu_context.circuit_bootstrap_raw(enc.reshape(3 * 128, 1, BIG), ident).reshape(3, 128, BIG)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
    ek2 = aes_var.key_schedule_plain(KEY2)
    assert _bytes_of(client, got) == b"".join(aes_var.encrypt_block_plain(ek2, b, 2) for b in blocks)


def test_masks_equal_numpy(gpu_context, tweaks2):
    torch = pytest.importorskip("torch")
    unit_of = [i % 2 for i in range(len(INDICES))]
    got = V.xts_masks_raw(gpu_context, tweaks2, unit_of, INDICES)
    assert np.array_equal(got, _masks_np(tweaks2, unit_of, INDICES))
    d_t = torch.from_numpy(tweaks2.view(np.int64)).to("cuda:0")
    d_m = torch.full((len(INDICES), 128, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.xts_masks_device(gpu_context, d_t.data_ptr(), 2, unit_of, INDICES, d_m.data_ptr())
    assert np.array_equal(d_m.cpu().numpy().view(np.uint64), got)
    assert _code(lambda: V.xts_masks_raw(gpu_context, tweaks2, [0, 2], [0, 1])) == N.TAE_E_ARG


def test_transcipher_equals_composition(gpu_context, client, keys128, tweaks2):
    dk1, rk2 = keys128
    data_a, data_b = bytes((29 * i + 5) & 255 for i in range(32)), bytes((13 * i + 1) & 255 for i in range(16))
    got = V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, data_a), (7, data_b, 127)], rounds=2)
    assert got.shape == (48, 8, BIG)
    masks = V.xts_masks_raw(gpu_context, tweaks2, [0, 0, 1], [0, 1, 127])
    blocks = _trivial_blocks([data_a[:16], data_a[16:], data_b]) + masks
    want = V.decrypt_blocks_raw(gpu_context, dk1, blocks, 2) + masks
    assert np.array_equal(got.reshape(3, 128, BIG), want)


def test_masks_shared_lists(gpu_context, tweaks2):
    """The lists of index 5 are read under two bases and twice under one; beside them index 0, whose lists all have
    width 1."""
    torch = pytest.importorskip("torch")
    unit_of, index = [0, 1, 0, 1, 1], [5, 5, 5, 0, 5]
    got = V.xts_masks_raw(gpu_context, tweaks2, unit_of, index)
    assert np.array_equal(got, _masks_np(tweaks2, unit_of, index))
    d_t = torch.from_numpy(tweaks2.view(np.int64)).to("cuda:0")
    d_m = torch.full((len(index), 128, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.xts_masks_device(gpu_context, d_t.data_ptr(), 2, unit_of, index, d_m.data_ptr())
    assert np.array_equal(d_m.cpu().numpy().view(np.uint64), got)


@pytest.fixture(scope="module")
def three_blocks(gpu_context, keys128):
    """The units of test_transcipher_equals_composition and their words from host arrays."""
    units = [(UNIT, bytes((29 * i + 5) & 255 for i in range(32))), (7, bytes((13 * i + 1) & 255 for i in range(16)), 127)]
    return units, V.xts_transcipher_raw(gpu_context, keys128[0], keys128[1], units, rounds=2)


def test_chunked_transcipher_gives_the_same_words(product_raw, keys128, three_blocks, monkeypatch):
    """Three blocks in chunks of 2: two mask plans are alive in one call, and the first unit's tweak is shared across
    the boundary.  The chunk size is read when the context is created."""
    monkeypatch.setenv("TAE_CTR_CHUNK_BLOCKS", "2")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_CTR_CHUNK_BLOCKS")
    units, want = three_blocks
    assert np.array_equal(V.xts_transcipher_raw(ctx2, keys128[0], keys128[1], units, rounds=2), want)
    del ctx2


def test_transcipher_device_memory(gpu_context, keys128, three_blocks):
    torch = pytest.importorskip("torch")
    units, want = three_blocks
    d_dk1, d_rk2 = (torch.from_numpy(k.view(np.int64)).to("cuda:0") for k in keys128)
    d_out = torch.full((48, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.xts_transcipher_device(gpu_context, 128, d_dk1.data_ptr(), d_rk2.data_ptr(), units, 2, d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)


def test_ieee_vector_ten_rounds(gpu_context, client):
    """Vector 2 with both key schedules and the decryption key made under FHE; raw arrays, then handles and pack."""
    k1 = client.encrypt_bits_raw(_bits(KEY1), start_index=7_020_000)
    k2 = client.encrypt_bits_raw(_bits(KEY2), start_index=7_021_000)
    rk1, rk2 = V.key_schedule_raw(gpu_context, k1), V.key_schedule_raw(gpu_context, k2)
    dk1 = V.decrypt_key_raw(gpu_context, rk1)
    out = V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, CT)])
    assert _bytes_of(client, out) == PT
    handles = [[gpu_context.bit_from_data(k[i], 1) for i in range(44 * W)] for k in (dk1, rk2)]
    res = gpu_context.pack(V.xts_transcipher(gpu_context, handles[0], handles[1], [(UNIT, CT)]))
    assert res.origin == "server" and res.count == 256
    assert aes_128.decrypt_byte_array_packed(client, res) == PT


def test_xts_256_one_block(gpu_context, client):
    key1, key2 = bytes(range(32)), bytes(range(0x40, 0x60))
    rk1 = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(key1))), start_index=7_030_000)
    rk2 = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(key2))), start_index=7_040_000)
    dk1 = V.decrypt_key_raw(gpu_context, rk1)
    tweak = bytes(range(0xF0, 0x100))
    msg = bytes((17 * i + 9) & 255 for i in range(16))
    data = aes_var.xts_encrypt_plain(key1, key2, tweak, msg, first_block=1)
    out = V.xts_transcipher_raw(gpu_context, dk1, rk2, [(tweak, data, 1)])
    assert out.shape == (16, 8, BIG)
    assert _bytes_of(client, out) == aes_var.xts_decrypt_plain(key1, key2, tweak, data, first_block=1) == msg


def test_bitct_levels_and_ids(gpu_context, client, keys128):
    dk1, rk2 = ([gpu_context.bit_from_data(k[i], 1) for i in range(44 * W)] for k in keys128)
    units = [(UNIT, bytes(32)), (7, bytes(16), 127)]
    out = V.xts_transcipher(gpu_context, dk1, rk2, units, rounds=1)
    assert len(out) == 48
    for blk, j in enumerate((0, 1, 127)):
        rows = _mask_rows(j)
        levels = [b.noise_level_squared for byte in out[16 * blk:16 * blk + 16] for b in byte]
        assert levels == [9 + len(r) for r in rows]
        assert max(levels) == 9 + aes_var.xts_row_weight(j)
    # coefficient 9 of alpha T reads coefficient 8 of T: ciphertext 14 of block 1 and ciphertext 15 of block 0 share
    # tweak ciphertext 15, at different places of the block, so the key bits they carry differ
    assert 15 in _mask_rows(1)[14] and _mask_rows(0)[15] == [15]
    with pytest.raises(tfhe_aes.NoiseNotIndependent):
        out[1][7].clone().__ixor__(out[16 + 1][6])
    other = out[1][7].clone()
    other ^= out[32 + 1][6]  # the same places, another data unit: no tweak bit in common
    assert other.noise_level_squared == 10 + 9 + len(_mask_rows(127)[14])


def test_range_equals_whole(gpu_context, keys128):
    dk1, rk2 = keys128
    data = bytes((31 * i + 7) & 255 for i in range(48))
    whole = V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, data)], rounds=1)
    part = V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, data[16:], 1)], rounds=1)
    assert part.shape == (32, 8, BIG)
    assert np.array_equal(part, whole[16:])


def test_param_errors(gpu_context, gpu_context8, keys128):
    dk1, rk2 = keys128
    gpu_context.set_timing(True)
    try:
        V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, bytes(16))], rounds=1)
        before = gpu_context.last_stage_times()
        assert before["pbs_launches"] > 0
        assert _code(lambda: V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, bytes(17))])) == N.TAE_E_PARAM
        assert _code(lambda: V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, b"")])) == N.TAE_E_PARAM
        assert _code(lambda: V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, bytes(32), 65534)])) == N.TAE_E_NOISE
        assert gpu_context.last_stage_times() == before
    finally:
        gpu_context.set_timing(False)
    assert _code(lambda: V.xts_transcipher_raw(gpu_context, dk1, rk2, [(UNIT, bytes(16))], rounds=11)) == N.TAE_E_PARAM
    L8 = gpu_context8.lwe_size
    k8 = np.zeros((44 * W, L8), dtype=np.uint64)
    assert _code(lambda: V.xts_transcipher_raw(gpu_context8, k8, k8, [(UNIT, bytes(16))])) == N.TAE_E_PARAM
    assert _code(lambda: V.xts_tweaks_raw(gpu_context8, k8, [UNIT])) == N.TAE_E_PARAM
