"""AES-CCM decryption of public frames on the GPU (tae_aesx_ccm_*, tae_aesm_ccm_*, tae_aesm_pub_keystream_raw;
RFC 3610; the reference has no CCM).

Word-for-word anchors.  The pipeline is deterministic in its input ciphertexts, so
- the public-block pass must equal the existing block cipher on trivial encryptions of the blocks,
- the payload bits and the tag difference must equal a chain rebuilt here from the existing block cipher alone:
  I_0 = trivial(B_0), Xk_t = encrypt_blocks_raw(I_t), and I_t / the difference from the formulas of DESIGN.md
  5.13 in numpy uint64 (encrypt_blocks_raw adds round key 0 itself, so I_t is the step's state without it),
- every frame of a ragged multi-key batch must equal its single-frame call.
Full round counts are checked through decryption against RFC 3610 packet vector 1 and the plain model.
"""
import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_multi, aes_var

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
V = aes_var.GalMulAes
M = aes_multi.GalMulAesMulti
W = 32
# RFC 3610 packet vector 1
KEY = bytes(range(0xC0, 0xD0))
NONCE = bytes.fromhex("00000003020100A0A1A2A3A4A5")
AAD = bytes(range(8))
PAYLOAD = bytes(range(8, 0x1F))
FRAME = bytes.fromhex("588C979A61C663D2F066D0C2C0F989806D5F6B61DAC38417E8D12CFDF926E0")
KEYS256 = (bytes(range(32)), bytes(range(0x40, 0x60)))


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _bytes_of(client, cts):
    bits = client.decrypt_bits_raw(cts.reshape(-1, cts.shape[-1])).reshape(-1, 8)
    return bytes(aes_128.bits_to_u8(b) for b in bits)


def _trivial(data):
    """[len][8][BIG] trivial encryptions of bytes."""
    cts = np.zeros((len(data), 8, BIG), dtype=np.uint64)
    cts[:, :, -1] = np.array(_bits(data), dtype=np.uint64).reshape(-1, 8) << np.uint64(63)
    return cts


def _trivial_blocks(blocks):
    return _trivial(b"".join(bytes(b) for b in blocks)).reshape(len(blocks), 128, BIG)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def keys(client):
    """Fresh encryptions of plain expanded keys: vector 1's, and a table of two 32-byte keys."""
    rk = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(KEY))), start_index=8_000_000)
    table = np.stack([client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(k))),
                                              start_index=8_010_000 + 10_000 * s) for s, k in enumerate(KEYS256)])
    return rk, table


def _chain_np(ctx, rk, nonce, aad, data, tag_len, rounds):
    """The payload bits and the tag difference from existing entry points and numpy sums."""
    nr = rk.shape[0] // 128 - 1
    body, tag = data[:len(data) - tag_len], data[len(data) - tag_len:]
    ctr, mac, src = aes_var.ccm_format(nonce, aad, len(body), tag_len)
    s = V.encrypt_blocks_raw(ctx, rk, _trivial_blocks(ctr), rounds)
    plain = s[1:].reshape(-1, 8, BIG)[:len(body)] + _trivial(body)
    rk_last = rk[128 * nr:128 * nr + 128]
    xk = V.encrypt_blocks_raw(ctx, rk, _trivial_blocks(mac[:1]), rounds)[0]
    for t in range(1, len(mac)):
        state = xk.copy()
        for pos in range(16):
            rows = slice(8 * pos, 8 * pos + 8)
            if src[t, pos] >= 0:
                state[rows] += plain[src[t, pos]] - np.uint64(2) * rk_last[rows]
            else:
                state[rows] += _trivial(bytes([mac[t, pos]]))[0]
        xk = V.encrypt_blocks_raw(ctx, rk, state[None], rounds)[0]
    n = 8 * tag_len
    diff = xk[:n] + s[0, :n] - np.uint64(2) * rk_last[:n] + _trivial(tag).reshape(n, BIG)
    return plain, diff.reshape(tag_len, 8, BIG)


def test_pass1_equals_trivial_blocks(gpu_context, keys):
    rk, table = keys
    ctr, mac, _ = aes_var.ccm_format(NONCE, AAD, len(PAYLOAD), 8)
    blocks = [bytes(b) for b in ctr] + [bytes(mac[0])]
    got = V.public_keystream_raw(gpu_context, rk, blocks, rounds=2)
    assert got.shape == (4, 128, BIG)
    assert np.array_equal(got, V.encrypt_blocks_raw(gpu_context, rk, _trivial_blocks(blocks), 2))
    slots = [1, 0, 0, 1]
    got2 = M.public_keystream_raw(gpu_context, table, slots, blocks, rounds=2)
    want2 = M.encrypt_blocks_raw(gpu_context, table, slots, _trivial_blocks(blocks), 2)
    assert np.array_equal(got2, want2)
    assert not np.array_equal(got2[1], got2[3])


def test_chain_equals_composition(gpu_context, client, keys):
    torch = pytest.importorskip("torch")
    rk, _ = keys
    plain, diff = V.ccm_transcipher_raw(gpu_context, rk, NONCE, AAD, FRAME, 8, rounds=2)
    assert plain.shape == (23, 8, BIG) and diff.shape == (8, 8, BIG)
    want_plain, want_diff = _chain_np(gpu_context, rk, NONCE, AAD, FRAME, 8, 2)
    assert np.array_equal(plain, want_plain)
    assert np.array_equal(diff, want_diff)
    model = aes_var.ccm_decrypt_plain(KEY, NONCE, AAD, FRAME, 8, rounds=2)
    assert (_bytes_of(client, plain), _bytes_of(client, diff)) == model
    # device pointers: the same words
    d_rk = torch.from_numpy(rk.view(np.int64)).to("cuda:0")
    d_out = torch.full((23, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    d_diff = torch.full((8, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.ccm_transcipher_device(gpu_context, 128, d_rk.data_ptr(), NONCE, AAD, FRAME, 8, 2, d_out.data_ptr(),
                             d_diff.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), plain)
    assert np.array_equal(d_diff.cpu().numpy().view(np.uint64), diff)


def _ragged_frames():
    """Three frames of 3, 3 and 4 MAC blocks under two 32-byte keys, L = 2 and L = 8: (streams, payloads)."""
    n13, n7 = bytes(range(0x10, 0x1D)), bytes(range(0x30, 0x37))
    shapes = [(1, n13, b"", bytes((7 * i + 3) & 255 for i in range(17))),
              (0, n7, bytes(range(0x50, 0x5F)), b""),
              (1, n7, bytes(range(8)), bytes((11 * i + 1) & 255 for i in range(23)))]
    streams = [(slot, nonce, aad, aes_var.ccm_encrypt_plain(KEYS256[slot], nonce, aad, pt, 6, rounds=2))
               for slot, nonce, aad, pt in shapes]
    return streams, [pt for _, _, _, pt in shapes]


@pytest.fixture(scope="module")
def ragged(gpu_context, keys):
    return M.ccm_transcipher_raw(gpu_context, keys[1], _ragged_frames()[0], 6, rounds=2)


def test_ragged_batch_equals_single_frames(gpu_context, client, keys, ragged):
    """The chain runs the frames longest first and returns them in the caller's order."""
    _, table = keys
    streams, payloads = _ragged_frames()
    assert [g[0].shape[0] for g in ragged] == [17, 0, 23]
    for (slot, nonce, aad, data), (plain, diff), payload in zip(streams, ragged, payloads):
        one_plain, one_diff = V.ccm_transcipher_raw(gpu_context, table[slot], nonce, aad, data, 6, rounds=2)
        assert np.array_equal(plain, one_plain)
        assert np.array_equal(diff, one_diff)
        assert _bytes_of(client, plain) == payload and aes_var.ccm_tag_ok(client, diff)


def test_chunked_pass_gives_the_same_words(product_raw, keys, ragged, monkeypatch):
    """The 10 public blocks of the ragged batch (A_1 A_2 A_0 B_0 | A_0 B_0 | A_1 A_2 A_0 B_0) in chunks of 3: the
    boundaries fall inside the kept pair A_0 / B_0 of two frames and between frames, and the last chunk has no
    payload block.  The chunk size is read when the context is created."""
    monkeypatch.setenv("TAE_CTR_CHUNK_BLOCKS", "3")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_CTR_CHUNK_BLOCKS")
    got = M.ccm_transcipher_raw(ctx2, keys[1], _ragged_frames()[0], 6, rounds=2)
    for (plain, diff), (want_plain, want_diff) in zip(got, ragged):
        assert np.array_equal(plain, want_plain) and np.array_equal(diff, want_diff)
    del ctx2


def test_vector_1_full_rounds(gpu_context, client):
    """The key schedule made under FHE; the authentic frame, a flipped tag bit and a flipped ciphertext bit."""
    k = client.encrypt_bits_raw(_bits(KEY), start_index=8_040_000)
    rk = V.key_schedule_raw(gpu_context, k)
    plain, diff = V.ccm_transcipher_raw(gpu_context, rk, NONCE, AAD, FRAME, 8)
    assert _bytes_of(client, plain) == PAYLOAD
    assert aes_var.ccm_tag_ok(client, diff)
    for at in (len(FRAME) - 3, 5):  # a tag byte, a ciphertext byte
        bad = bytearray(FRAME)
        bad[at] ^= 0x10
        want_plain, want_diff = aes_var.ccm_decrypt_plain(KEY, NONCE, AAD, bytes(bad), 8)
        assert any(want_diff)
        plain, diff = V.ccm_transcipher_raw(gpu_context, rk, NONCE, AAD, bytes(bad), 8)
        assert _bytes_of(client, plain) == want_plain
        assert _bytes_of(client, diff) == want_diff
        assert not aes_var.ccm_tag_ok(client, diff)


def test_aes256_frame_fourteen_rounds(gpu_context, client, keys):
    _, table = keys
    nonce, aad, msg = bytes(range(0x20, 0x2B)), bytes(range(5)), bytes((19 * i + 2) & 255 for i in range(9))
    data = aes_var.ccm_encrypt_plain(KEYS256[0], nonce, aad, msg, 16)
    plain, diff = V.ccm_transcipher_raw(gpu_context, table[0], nonce, aad, data, 16)
    assert diff.shape == (16, 8, BIG)
    assert _bytes_of(client, plain) == msg and aes_var.ccm_tag_ok(client, diff)


def test_bitct_frame_packed(gpu_context, client, keys):
    """Handles: the levels and ids of DESIGN.md 5.13, then both results through FheContext.pack."""
    rk, _ = keys
    ek = [gpu_context.bit_from_data(rk[i], 1) for i in range(44 * W)]
    msg = bytes((23 * i + 4) & 255 for i in range(5))
    data = aes_var.ccm_encrypt_plain(KEY, NONCE, b"", msg, 4)
    bits, diff = V.ccm_transcipher(gpu_context, ek, NONCE, b"", data, 4)
    assert len(bits) == 5 and len(diff) == 4
    assert {b.noise_level_squared for byte in bits for b in byte} == {9}
    assert {b.noise_level_squared for byte in diff for b in byte} == {16}
    x = diff[0][0].clone()
    x ^= diff[0][1]  # two tag-difference bits of one frame
    x ^= bits[1][0]  # and a payload bit of another position
    assert x.noise_level_squared == 16 + 16 + 9
    packed = gpu_context.pack(bits)
    assert packed.origin == "server" and packed.count == 40
    assert aes_128.decrypt_byte_array_packed(client, packed) == msg
    assert aes_var.ccm_tag_ok(client, gpu_context.pack(diff)) and aes_var.ccm_tag_ok(client, diff)


def test_param_errors(gpu_context, gpu_context8, keys):
    rk, _ = keys
    gpu_context.set_timing(True)
    try:
        V.ccm_transcipher_raw(gpu_context, rk, NONCE, b"", bytes(4), 4, rounds=2)
        before = gpu_context.last_stage_times()
        assert before["pbs_launches"] > 0
        for call in (lambda: V.ccm_transcipher_raw(gpu_context, rk, bytes(6), AAD, FRAME, 8),
                     lambda: V.ccm_transcipher_raw(gpu_context, rk, bytes(14), AAD, FRAME, 8),
                     lambda: V.ccm_transcipher_raw(gpu_context, rk, NONCE, AAD, FRAME, 7),
                     lambda: V.ccm_transcipher_raw(gpu_context, rk, NONCE, AAD, FRAME[:7], 8),
                     lambda: V.ccm_transcipher_raw(gpu_context, rk, NONCE, AAD, FRAME, 8, rounds=1)):
            assert _code(call) == N.TAE_E_PARAM
        assert gpu_context.last_stage_times() == before
    finally:
        gpu_context.set_timing(False)
    k8 = np.zeros((44 * W, gpu_context8.lwe_size), dtype=np.uint64)
    assert _code(lambda: V.ccm_transcipher_raw(gpu_context8, k8, NONCE, AAD, FRAME, 8)) == N.TAE_E_PARAM
    assert _code(lambda: V.public_keystream_raw(gpu_context8, k8, [bytes(16)])) == N.TAE_E_PARAM
