"""Segmented GHASH on the GPU (tae_aesx_ghash_stride_key*, tae_aesx_gcm_long_transcipher*; the
reference has no GCM).

Word-for-word anchors, as tests/test_gpu_gcm.py: the pipeline is deterministic in its input ciphertexts, so the stride
key and the long call must equal compositions of existing public entry points (public_keystream_raw,
circuit_bootstrap_raw, gf128_square_raw, gf128_product_raw, gcm_transcipher_raw) and numpy u64 row sums over the plans
restated in tests/gcm_long_ref.py.  Where the cipher takes part in such a comparison it runs 2 rounds.  Power tables and
stride keys are fresh client-side encryptions of the plain powers unless a test is about making them.
"""
import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var
from tests import gcm_ref as R
from tests.gcm_long_ref import inner_chunks, long_plan, n_segments

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
V = aes_var.GalMulAes
W = 32
KEY256 = bytes(range(32))
_AT = [60_000_000]  # every client-made array has an index range of its own


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _enc(client, data):
    out = client.encrypt_bits_raw(_bits(data), start_index=_AT[0])
    _AT[0] += 100_000
    return out


def _bytes_of(client, cts):
    bits = client.decrypt_bits_raw(cts.reshape(-1, cts.shape[-1])).reshape(-1, 8)
    return bytes(aes_128.bits_to_u8(b) for b in bits)


def _trivial(data):
    cts = np.zeros((len(data), 8, BIG), dtype=np.uint64)
    cts[:, :, -1] = np.array(_bits(data), dtype=np.uint64).reshape(-1, 8) << np.uint64(63)
    return cts


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def _powers(h, n):
    out, p = [], h
    for _ in range(n):
        out.append(p)
        p = R.mul(p, h)
    return out


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def lut_id(gpu_context):
    return gpu_context.generate_lookup_table(1, 1, lambda v: v)


def _refresh(ctx, lut_id, cts):
    """The identity bootstrap of [n][BIG] through the public circuit bootstrap."""
    return ctx.circuit_bootstrap_raw(cts.reshape(-1, 1, BIG), lut_id).reshape(-1, BIG)


def _tables(client, key, rounds, n_powers, seg, n_strides):
    """(rk, hk, sk) as fresh encryptions of the plain expanded key, H^1 .. H^n_powers and H^seg .. H^(n_strides seg)."""
    ek = aes_var.key_schedule_plain(key)
    powers = _powers(aes_var.encrypt_block_plain(ek, bytes(16), rounds), max(n_powers, seg * n_strides))
    rk = _enc(client, b"".join(ek))
    hk = np.stack([_enc(client, q) for q in powers[:n_powers]])
    sk = np.stack([_enc(client, powers[seg * j - 1]) for j in range(1, n_strides + 1)])
    return rk, hk, sk


@pytest.fixture(scope="module")
def two(client):
    """Test case 3's key at 2 rounds: a table of 4 powers, the stride key of seg = 2 with 3 strides."""
    return _tables(client, R.KEY3, 2, 4, 2, 3)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


# ---- 1. the stride key ------------------------------------------------------------------------------------------------
def test_stride_key_equals_squares_and_products(gpu_context, client, two):
    torch = pytest.importorskip("torch")
    _, hk, _ = two
    sk = V.ghash_stride_key_raw(gpu_context, hk[:2], 2, 3)
    assert sk.shape == (3, 128, BIG)
    assert np.array_equal(sk[0], hk[1])
    assert np.array_equal(sk[1], V.gf128_square_raw(gpu_context, sk[:1])[0])
    assert np.array_equal(sk[2], V.gf128_product_raw(gpu_context, sk[1:2], sk[:1])[0])
    h = aes_var.encrypt_block_plain(aes_var.key_schedule_plain(R.KEY3), bytes(16), 2)
    assert [_bytes_of(client, t) for t in sk] == _powers(h, 6)[1::2]
    d_hk = _dev(torch, hk[:2])
    d_sk = torch.full((3, 128, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.ghash_stride_key_device(gpu_context, d_hk.data_ptr(), 2, 2, 3, d_sk.data_ptr())
    assert np.array_equal(d_sk.cpu().numpy().view(np.uint64), sk)


def test_ghash_key_keeps_its_words(gpu_context, two, lut_id):
    """The generation loop ghash_key now shares with the stride key: H^1 the refreshed E(0), H^2 its square, H^3 the
    product H^2 H^1, H^4 the square of H^2, from public entry points."""
    rk = two[0]
    hk = V.ghash_key_raw(gpu_context, rk, 4, rounds=2)
    h1 = _refresh(gpu_context, lut_id, V.public_keystream_raw(gpu_context, rk, [bytes(16)], 2)[0])
    h2 = V.gf128_square_raw(gpu_context, h1[None])[0]
    h3 = V.gf128_product_raw(gpu_context, h2[None], h1[None])[0]
    h4 = V.gf128_square_raw(gpu_context, h2[None])[0]
    assert np.array_equal(hk, np.stack([h1, h2, h3, h4]))


# ---- 2. short frames are the old call -----------------------------------------------------------------------------------
def test_short_frame_equals_the_single_table_call(gpu_context, two):
    rk, hk, sk = two
    aad, msg = bytes(range(8)), bytes((13 * i + 7) & 255 for i in range(20))  # m = 4
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, aad, msg, 12, rounds=2)
    (plain, diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 4, [(R.IV3, aad, data)], 12, rounds=2)
    (old_plain, old_diff), = V.gcm_transcipher_raw(gpu_context, rk, hk, [(R.IV3, aad, data)], 12, rounds=2)
    assert np.array_equal(plain, old_plain) and np.array_equal(diff, old_diff)


# ---- 3. composition ---------------------------------------------------------------------------------------------------
def _long_np(ctx, lut_id, rk, hk, sk, seg, iv, aad, data, tag_len, rounds):
    """The payload bits and the tag difference of one frame from public_keystream_raw, the given tables, numpy row
    sums, the identity bootstrap and gf128_product_raw."""
    c, tag = data[:len(data) - tag_len], data[len(data) - tag_len:]
    n_blk = (len(c) + 15) // 16
    s = V.public_keystream_raw(ctx, rk, [iv + (1 + i).to_bytes(4, "big") for i in range(n_blk + 1)], rounds)
    plain = s[1:].reshape(-1, 8, BIG)[:len(c)] + _trivial(c)
    tb = min(seg, len(R.hashed_blocks(aad, c)))
    table = hk[:tb].reshape(-1, BIG)
    inner, final = long_plan(aad, c, tag_len, seg)
    products = []
    for j, rows in enumerate(inner):
        chunk_rows, of_row = [], []
        for row in rows:
            cs = inner_chunks(row)
            of_row.append(list(range(len(chunk_rows), len(chunk_rows) + len(cs))))
            chunk_rows += cs
        fresh = _refresh(ctx, lut_id, R.sum_rows(table, chunk_rows))
        s_c = _refresh(ctx, lut_id, R.sum_rows(fresh, of_row))
        products.append(V.gf128_product_raw(ctx, s_c[None], sk[j][None])[0])
    src = np.concatenate([table, s[0]] + products)
    chunk_rows, of_row = [], []
    for r, row in enumerate(final):
        cs = R.row_chunks(row)
        cs[0] = [128 * tb + r] + cs[0]
        of_row.append(list(range(len(chunk_rows), len(chunk_rows) + len(cs))))
        chunk_rows += cs
    fresh = _refresh(ctx, lut_id, R.sum_rows(src, chunk_rows))
    diff = R.sum_rows(fresh, of_row) + _trivial(tag).reshape(-1, BIG)
    return plain, diff.reshape(tag_len, 8, BIG)


COMP_AAD, COMP_MSG = bytes(range(8)), bytes((29 * i + 11) & 255 for i in range(40))  # m = 5; seg = 2: C = 3


def test_three_segments_equal_the_composition(gpu_context, client, lut_id, two):
    torch = pytest.importorskip("torch")
    rk, hk, sk = two
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, COMP_AAD, COMP_MSG, 12, rounds=2)
    assert n_segments(len(R.hashed_blocks(COMP_AAD, COMP_MSG)), 2) == 3
    (plain, diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 2, [(R.IV3, COMP_AAD, data)], 12, rounds=2)
    assert plain.shape == (40, 8, BIG) and diff.shape == (12, 8, BIG)
    want_plain, want_diff = _long_np(gpu_context, lut_id, rk, hk, sk, 2, R.IV3, COMP_AAD, data, 12, 2)
    assert np.array_equal(plain, want_plain)
    assert np.array_equal(diff, want_diff)
    assert _bytes_of(client, plain) == COMP_MSG
    assert _bytes_of(client, diff) == bytes(12) and aes_var.gcm_tag_ok(client, diff)
    assert aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, COMP_AAD, data, 12, rounds=2) == (COMP_MSG, bytes(12))
    d_rk, d_hk, d_sk = _dev(torch, rk), _dev(torch, hk), _dev(torch, sk)
    d_out = torch.full((40, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    d_diff = torch.full((12, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.gcm_long_transcipher_device(gpu_context, 128, d_rk.data_ptr(), d_hk.data_ptr(), 4, d_sk.data_ptr(), 3, 2,
                                  [(R.IV3, COMP_AAD, data)], 12, 2, d_out.data_ptr(), d_diff.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), plain)
    assert np.array_equal(d_diff.cpu().numpy().view(np.uint64), diff)
    # one received-tag bit flipped: the plain model's difference
    bad = bytearray(data)
    bad[-3] ^= 0x10
    (_, bad_diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 2, [(R.IV3, COMP_AAD, bytes(bad))], 12, rounds=2)
    want = aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, COMP_AAD, bytes(bad), 12, rounds=2)[1]
    assert any(want) and _bytes_of(client, bad_diff) == want and not aes_var.gcm_tag_ok(client, bad_diff)


def test_table_and_stride_key_are_read_in_place(gpu_context, two):
    """seg = 2 and m = 5: the inner and the final chunk sums read the table's first two blocks where the caller keeps
    them.  Blocks 2..3 enter no output word, and neither the table nor the stride key is written."""
    torch = pytest.importorskip("torch")
    rk, hk, sk = two
    frames = [(R.IV3, COMP_AAD, aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, COMP_AAD, COMP_MSG, 12, rounds=2))]
    (plain, diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 2, frames, 12, rounds=2)
    scribbled = hk.copy()
    scribbled[2:] = (np.arange(scribbled[2:].size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(scribbled[2:].shape)
    (plain2, diff2), = V.gcm_long_transcipher_raw(gpu_context, rk, scribbled, sk, 2, frames, 12, rounds=2)
    assert np.array_equal(plain2, plain) and np.array_equal(diff2, diff)
    d_rk, d_hk, d_sk = _dev(torch, rk), _dev(torch, scribbled), _dev(torch, sk)
    d_out = torch.full((40, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    d_diff = torch.full((12, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.gcm_long_transcipher_device(gpu_context, 128, d_rk.data_ptr(), d_hk.data_ptr(), 4, d_sk.data_ptr(), 3, 2, frames, 12,
                                  2, d_out.data_ptr(), d_diff.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), plain)
    assert np.array_equal(d_diff.cpu().numpy().view(np.uint64), diff)
    assert np.array_equal(d_hk.cpu().numpy().view(np.uint64), scribbled)
    assert np.array_equal(d_sk.cpu().numpy().view(np.uint64), sk)


def test_rows_without_a_source(gpu_context, client, lut_id, two):
    """seg = 1 and an all-zero ciphertext block: every inner row of that segment is one empty chunk, the zero
    ciphertext through rowsum_kernel and the identity bootstrap.  At seg = 1 the stride key is the table."""
    rk, hk, _ = two
    c = bytes(16) + bytes((17 * i + 9) & 255 for i in range(16))
    pt = aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, b"", c + bytes(12), 12, rounds=2)[0]
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, b"", pt, 12, rounds=2)
    assert data[:32] == c
    src, chunks = aes_var.gcm_long_rows(R.IV3, b"", c, 12, 1, 1, 2)
    assert src.shape == (3, 128) and not src[2].any() and set(chunks[2]) == {1}  # exponent 3 is the zero block
    sk = hk[:2].copy()
    (plain, diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk[:1], sk, 1, [(R.IV3, b"", data)], 12, rounds=2)
    want_plain, want_diff = _long_np(gpu_context, lut_id, rk, hk[:1], sk, 1, R.IV3, b"", data, 12, 2)
    assert np.array_equal(plain, want_plain) and np.array_equal(diff, want_diff)
    assert _bytes_of(client, plain) == pt and aes_var.gcm_tag_ok(client, diff)


# ---- 4. a ragged batch ------------------------------------------------------------------------------------------------
def _ragged():
    iv_b = bytes(range(0x20, 0x2C))
    shapes = [(R.IV3, b"", bytes((7 * i + 3) & 255 for i in range(9))),        # m = 2: C = 1
              (iv_b, bytes(range(15)), bytes((5 * i + 1) & 255 for i in range(32))),  # m = 4: C = 2
              (R.IV3, COMP_AAD, COMP_MSG)]                                           # m = 5: C = 3
    return shapes, [(iv, aad, aes_var.gcm_encrypt_plain(R.KEY3, iv, aad, pt, 8, rounds=2)) for iv, aad, pt in shapes]


def test_ragged_batch_equals_single_frames(gpu_context, product_raw, client, two, monkeypatch):
    rk, hk, sk = two
    shapes, frames = _ragged()
    assert [n_segments(len(R.hashed_blocks(aad, pt)), 2) for _, aad, pt in shapes] == [1, 2, 3]
    got = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 2, frames, 8, rounds=2)
    assert [g[0].shape[0] for g in got] == [9, 32, 40]
    for frame, (plain, diff), (_, _, pt) in zip(frames, got, shapes):
        (one_plain, one_diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 2, [frame], 8, rounds=2)
        assert np.array_equal(plain, one_plain)
        assert np.array_equal(diff, one_diff)
        assert _bytes_of(client, plain) == pt and aes_var.gcm_tag_ok(client, diff)
    # the three inner segments in batches of 2 and 1, the public blocks in chunks of 3: read at context creation
    monkeypatch.setenv("TAE_GCM_SEG_BATCH", "2")
    monkeypatch.setenv("TAE_CTR_CHUNK_BLOCKS", "3")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_GCM_SEG_BATCH")
    monkeypatch.delenv("TAE_CTR_CHUNK_BLOCKS")
    again = V.gcm_long_transcipher_raw(ctx2, rk, hk, sk, 2, frames, 8, rounds=2)
    for (plain, diff), (want_plain, want_diff) in zip(again, got):
        assert np.array_equal(plain, want_plain) and np.array_equal(diff, want_diff)
    del ctx2


# ---- 5. past the old limit, full rounds -------------------------------------------------------------------------------
def test_hundred_blocks_full_rounds(gpu_context, client):
    rk, hk, sk = _tables(client, R.KEY3, 10, 31, 31, 3)
    # the frame test_gpu_gcm.py shows refused: 99 ciphertext blocks of 0xA5, here with its genuine tag
    pt = aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, b"", bytes([0xA5]) * (99 * 16) + bytes(16))[0]
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, b"", pt)
    assert data[:-16] == bytes([0xA5]) * (99 * 16)
    bad = bytearray(data)
    bad[5] ^= 0x10  # block 0: exponent 100, the top segment
    frames = [(R.IV3, b"", data), (R.IV3, b"", bytes(bad))]
    src, chunks = aes_var.gcm_long_rows(R.IV3, b"", data[:-16], 16, 31, 31, 3)
    assert src.shape == (4, 128) and src.max() <= 31 * 93 + 3 and chunks.max() <= 46
    got = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 31, frames, 16)
    assert _bytes_of(client, got[0][0]) == pt
    assert _bytes_of(client, got[0][1]) == bytes(16) and aes_var.gcm_tag_ok(client, got[0][1])
    want_plain, want_diff = aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, b"", bytes(bad))
    assert any(want_diff)
    assert _bytes_of(client, got[1][0]) == want_plain
    assert _bytes_of(client, got[1][1]) == want_diff and not aes_var.gcm_tag_ok(client, got[1][1])


# ---- 6. end to end under FHE-made keys --------------------------------------------------------------------------------
E2E_AAD, E2E_MSG = bytes(range(16)), bytes((41 * i + 5) & 255 for i in range(320))  # m = 22; seg = 8: C = 3


def test_end_to_end_fhe_made_keys(gpu_context, client):
    rk = V.key_schedule_raw(gpu_context, _enc(client, R.KEY3))
    hk = V.ghash_key_raw(gpu_context, rk, 8)
    sk = V.ghash_stride_key_raw(gpu_context, hk, 8, 2)
    h = aes_var.encrypt_block_plain(aes_var.key_schedule_plain(R.KEY3), bytes(16))
    assert [_bytes_of(client, t) for t in sk] == _powers(h, 16)[7::8]
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, E2E_AAD, E2E_MSG)
    assert n_segments(len(R.hashed_blocks(E2E_AAD, E2E_MSG)), 8) == 3
    (plain, diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 8, [(R.IV3, E2E_AAD, data)], 16)
    assert _bytes_of(client, plain) == E2E_MSG
    assert _bytes_of(client, diff) == bytes(16) and aes_var.gcm_tag_ok(client, diff)


def test_bitct_frame_packed(gpu_context, client):
    """Handles: the stride key's first entry clones the table's bits, later entries are fresh at level 1; payload bits
    at 9, a tag-difference bit at its chunk count; the legal XORs; both results through FheContext.pack."""
    key = _enc(client, R.KEY3)
    ek = V.key_schedule(gpu_context, [gpu_context.bit_from_data(key[i], 1) for i in range(128)])
    hk = V.ghash_key(gpu_context, ek, 8)
    sk = V.ghash_stride_key(gpu_context, hk, 8, 2)
    assert len(sk) == 2 * 128 and {b.noise_level_squared for b in sk} == {1}
    # entry 0 shares the ids of the table's block seg - 1, bit for bit; entry 1 is fresh
    x = sk[5].clone()
    assert _code(lambda: x.__ixor__(hk[7 * 128 + 5])) == N.TAE_E_INDEP
    x ^= hk[7 * 128 + 6]
    x ^= sk[128 + 5]
    x ^= hk[6 * 128 + 5]
    assert x.noise_level_squared == 4
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, E2E_AAD, E2E_MSG, 4)
    (bits, diff), = V.gcm_long_transcipher(gpu_context, ek, hk, sk, 8, [(R.IV3, E2E_AAD, data)], 4)
    assert len(bits) == 320 and len(diff) == 4
    assert {b.noise_level_squared for byte in bits for b in byte} == {9}
    _, chunks = aes_var.gcm_long_rows(R.IV3, E2E_AAD, data[:-4], 4, 8, 8, 2)
    _, final = long_plan(E2E_AAD, data[:-4], 4, 8)
    assert list(chunks[0, :32]) == [len(R.row_chunks(r)) for r in final] and max(chunks[0]) > 1
    assert [b.noise_level_squared for byte in diff for b in byte] == list(chunks[0, :32])
    x = diff[0][0].clone()
    x ^= diff[0][1]
    x ^= bits[1][0]
    assert x.noise_level_squared == int(chunks[0, 0]) + int(chunks[0, 1]) + 9
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(bits)) == E2E_MSG
    assert aes_var.gcm_tag_ok(client, gpu_context.pack(diff)) and aes_var.gcm_tag_ok(client, diff)


def test_aes256_frame_fourteen_rounds(gpu_context, client):
    rk, hk, sk = _tables(client, KEY256, 14, 2, 2, 2)
    iv, aad, msg = bytes(range(0x40, 0x4C)), bytes(range(5)), bytes((19 * i + 2) & 255 for i in range(41))  # m = 5
    data = aes_var.gcm_encrypt_plain(KEY256, iv, aad, msg, 13)
    (plain, diff), = V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 2, [(iv, aad, data)], 13)
    assert diff.shape == (13, 8, BIG)
    assert _bytes_of(client, plain) == msg and aes_var.gcm_tag_ok(client, diff)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stage_times(gpu_context, gpu_context8, two):
    rk, hk, sk = two
    tag = bytes(16)
    a5 = bytes([0xA5]) * (99 * 16) + tag
    long_call = V.gcm_long_transcipher_raw
    gpu_context.set_timing(True)
    try:
        long_call(gpu_context, rk, hk, sk, 2, [(R.IV3, b"", tag)], 16, rounds=2)
        before = gpu_context.last_stage_times()
        assert before["pbs_launches"] > 0
        zeros = lambda n: np.zeros((n, 128, BIG), dtype=np.uint64)  # never read: the refusal comes first
        for call in (lambda: long_call(gpu_context, rk, hk, sk, 0, [(R.IV3, b"", tag)], 16),
                     lambda: long_call(gpu_context, rk, hk, sk, 5, [(R.IV3, b"", tag)], 16),       # seg > n_powers
                     lambda: long_call(gpu_context, rk, zeros(128), sk, 65, [(R.IV3, b"", tag)], 16),  # seg > 64
                     lambda: long_call(gpu_context, rk, hk, zeros(0), 2, [(R.IV3, b"", tag)], 16),    # n_strides = 0
                     lambda: long_call(gpu_context, rk, hk, zeros(65), 2, [(R.IV3, b"", tag)], 16),
                     lambda: long_call(gpu_context, rk, zeros(31), zeros(2), 31, [(R.IV3, b"", a5)], 16),  # C - 1 = 3
                     lambda: long_call(gpu_context, rk, hk, sk, 2, [(R.IV3, b"", tag)], 16, rounds=1),
                     lambda: long_call(gpu_context, rk, hk, sk, 2, [(bytes(16), b"", tag)], 16),
                     lambda: long_call(gpu_context, rk, hk, sk, 2, [(R.IV3, b"", tag)], 5),
                     lambda: long_call(gpu_context, rk, hk, sk, 2, [(R.IV3, b"", tag[:7])], 8),
                     lambda: V.ghash_stride_key_raw(gpu_context, hk, 0, 2),
                     lambda: V.ghash_stride_key_raw(gpu_context, hk, 5, 2),
                     lambda: V.ghash_stride_key_raw(gpu_context, hk, 2, 0),
                     lambda: V.ghash_stride_key_raw(gpu_context, hk, 2, 65)):
            assert _code(call) == N.TAE_E_PARAM
        # 99 blocks of 0xA5 at seg = 48: rows of 48 * 93 sources
        assert _code(lambda: long_call(gpu_context, rk, zeros(48), zeros(64), 48, [(R.IV3, b"", a5)], 16)) == N.TAE_E_NOISE
        assert gpu_context.last_stage_times() == before
    finally:
        gpu_context.set_timing(False)
    k8 = np.zeros((44 * W, gpu_context8.lwe_size), dtype=np.uint64)
    h8 = np.zeros((1, 128, gpu_context8.lwe_size), dtype=np.uint64)
    assert _code(lambda: V.ghash_stride_key_raw(gpu_context8, h8, 1, 1)) == N.TAE_E_PARAM
    assert _code(lambda: long_call(gpu_context8, k8, h8, h8, 1, [(R.IV3, b"", tag)], 16)) == N.TAE_E_PARAM


# ---- 8. order ---------------------------------------------------------------------------------------------------------
def test_call_order(gpu_context, two):
    rk, hk, sk = two
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, COMP_AAD, COMP_MSG, 12, rounds=2)
    short = (R.IV3, bytes(range(8)), aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, bytes(range(8)), bytes(20), 12, rounds=2))
    others = (lambda: V.gf128_product_raw(gpu_context, hk[:1], hk[1:2]),
              lambda: np.concatenate([a.reshape(-1, BIG) for a in
                                      V.gcm_transcipher_raw(gpu_context, rk, hk, [short], 12, rounds=2)[0]]),
              lambda: V.ghash_key_raw(gpu_context, rk, 3, rounds=2))
    long_call = lambda: V.gcm_long_transcipher_raw(gpu_context, rk, hk, sk, 2, [(R.IV3, COMP_AAD, data)], 12, rounds=2)[0]
    before = [f() for f in others]
    first = long_call()
    after = [f() for f in others]
    second = long_call()
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
