"""AES-GCM decryption of public frames on the GPU (tae_aesx_ghash_key*, tae_aesx_gcm_transcipher*,
tae_stage_gf128_*; SP 800-38D; the reference has no GCM).

Word-for-word anchors.  The pipeline is deterministic in its input ciphertexts, so every stage must equal a
composition of existing public entry points (circuit_bootstrap_raw, public_keystream_raw) and numpy u64 row sums
over the plans restated in tests/gcm_ref.py.  Where the cipher takes part in such a comparison it runs 2 rounds.
Full round counts are checked through decryption against the GCM specification's test cases and the plain model.
"""
import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var
from tests import gcm_ref as R

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
V = aes_var.GalMulAes
W = 32
KEY256 = bytes(range(32))


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


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


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def lut_id(gpu_context):
    return gpu_context.generate_lookup_table(1, 1, lambda v: v)


def _refresh(ctx, lut_id, cts):
    """The identity bootstrap of [n][BIG] through the public circuit bootstrap."""
    return ctx.circuit_bootstrap_raw(cts.reshape(-1, 1, BIG), lut_id).reshape(-1, BIG)


def _elem(client, data, start):
    """[128][BIG] fresh encryptions of a field element: coefficient k at ciphertext k."""
    return client.encrypt_bits_raw(_bits(data), start_index=start)


@pytest.fixture(scope="module")
def rk2(client):
    """A fresh encryption of test case 3's plain expanded key, and the 2-round table of 4 powers under it."""
    return client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(R.KEY3))), start_index=9_000_000)


@pytest.fixture(scope="module")
def hk2(gpu_context, rk2):
    return V.ghash_key_raw(gpu_context, rk2, 4, rounds=2)


@pytest.fixture(scope="module")
def full(gpu_context, client):
    """Full rounds: the key schedule made under FHE, then the table of 8 powers (test case 4 hashes 7 blocks)."""
    rk = V.key_schedule_raw(gpu_context, client.encrypt_bits_raw(_bits(R.KEY3), start_index=9_020_000))
    return rk, V.ghash_key_raw(gpu_context, rk, 8)


# ---- the two field stages -------------------------------------------------------------------------------------------
def test_square_stage_equals_rowsums_and_refresh(gpu_context, client, lut_id):
    torch = pytest.importorskip("torch")
    a = [bytes((37 * i + 5) & 255 for i in range(16)), bytes([1]) + bytes(14) + bytes([1])]  # random; x^7 + x^127
    elems = np.stack([_elem(client, a[0], 9_030_000), _elem(client, a[1], 9_030_200)])
    got = V.gf128_square_raw(gpu_context, elems)
    want = np.stack([_refresh(gpu_context, lut_id, R.sum_rows(e, R.square_rows())) for e in elems])
    assert np.array_equal(got, want)
    for g, x in zip(got, a):
        assert _bytes_of(client, g) == R.mul(x, x)
    d_in = torch.from_numpy(elems.view(np.int64)).to("cuda:0")
    d_out = torch.full((2, 128, BIG), -1, dtype=torch.int64, device="cuda:0")
    N.check(N.lib().tae_stage_gf128_square(gpu_context._h, d_in.data_ptr(), 2, d_out.data_ptr(), N.TAE_MEM_DEVICE))
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), got)


def _product_np(ctx, lut_id, a, b):
    """The public path: big ciphertexts gathered, the 8 -> 7 circuit bootstrap, chunk sums, refresh, reduction, refresh."""
    ops = np.concatenate([a, b])
    pairs = np.stack([ops[R.pair_sources(g)] for g in range(1024)])
    lut = ctx.generate_lookup_table(8, 7, R.nibble_product)
    parts = ctx.circuit_bootstrap_raw(pairs, lut).reshape(1024 * 7, BIG)
    chunks, _, reduce, _ = R.product_plan()
    fresh = _refresh(ctx, lut_id, R.sum_rows(parts, chunks))
    return _refresh(ctx, lut_id, R.sum_rows(fresh, reduce))


def test_product_stage_equals_public_composition(gpu_context, client, lut_id):
    xa, xb = bytes((91 * i + 17) & 255 for i in range(16)), bytes((53 * i + 201) & 255 for i in range(16))
    top = bytes(15) + bytes([1])  # x^127
    a = np.stack([_elem(client, top, 9_040_000), _elem(client, xa, 9_040_200)])
    b = np.stack([_elem(client, top, 9_040_400), _elem(client, xb, 9_040_600)])
    one = V.gf128_product_raw(gpu_context, a[1:], b[1:])
    assert np.array_equal(one[0], _product_np(gpu_context, lut_id, a[1], b[1]))
    two = V.gf128_product_raw(gpu_context, a, b)
    assert np.array_equal(two[1], one[0])
    assert _bytes_of(client, two[1]) == R.mul(xa, xb)
    assert _bytes_of(client, two[0]) == R.mul(top, top)


# ---- the power table ------------------------------------------------------------------------------------------------
def test_ghash_key_powers_full_rounds(client, full):
    ek = aes_var.key_schedule_plain(R.KEY3)
    h = aes_var.encrypt_block_plain(ek, bytes(16))
    want, p = [], h
    for _ in range(8):
        want.append(p)
        p = R.mul(p, h)
    assert [_bytes_of(client, t) for t in full[1]] == want


def test_ghash_key_prefix_is_stable(gpu_context, rk2, hk2):
    assert np.array_equal(V.ghash_key_raw(gpu_context, rk2, 3, rounds=2), hk2[:3])


# ---- frames ---------------------------------------------------------------------------------------------------------
def _frame_np(ctx, lut_id, rk, hk, iv, aad, data, tag_len, rounds):
    """The payload bits and the tag difference from public_keystream_raw, the given table and numpy."""
    c, tag = data[:len(data) - tag_len], data[len(data) - tag_len:]
    n_blk = (len(c) + 15) // 16
    blocks = [iv + (1 + i).to_bytes(4, "big") for i in range(n_blk + 1)]
    s = V.public_keystream_raw(ctx, rk, blocks, rounds)
    plain = s[1:].reshape(-1, 8, BIG)[:len(c)] + _trivial(c)
    m = len(R.hashed_blocks(aad, c))
    src = np.concatenate([hk[:m].reshape(-1, BIG), s[0]])
    chunk_rows, of_row = [], []
    for r, row in enumerate(R.tag_rows(aad, c, tag_len)):
        cs = R.row_chunks(row)
        cs[0] = [128 * m + r] + cs[0]
        of_row.append(list(range(len(chunk_rows), len(chunk_rows) + len(cs))))
        chunk_rows += cs
    fresh = _refresh(ctx, lut_id, R.sum_rows(src, chunk_rows))
    diff = R.sum_rows(fresh, of_row) + _trivial(tag).reshape(-1, BIG)
    return plain, diff.reshape(tag_len, 8, BIG)


def test_single_frame_equals_composition(gpu_context, client, lut_id, rk2, hk2):
    torch = pytest.importorskip("torch")
    aad, msg = bytes(range(8)), bytes((13 * i + 7) & 255 for i in range(20))  # m = 4, a ragged last block
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, aad, msg, 12, rounds=2)
    (plain, diff), = V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(R.IV3, aad, data)], 12, rounds=2)
    assert plain.shape == (20, 8, BIG) and diff.shape == (12, 8, BIG)
    want_plain, want_diff = _frame_np(gpu_context, lut_id, rk2, hk2, R.IV3, aad, data, 12, 2)
    assert np.array_equal(plain, want_plain)
    assert np.array_equal(diff, want_diff)
    assert _bytes_of(client, plain) == msg and aes_var.gcm_tag_ok(client, diff)
    d_rk = torch.from_numpy(rk2.view(np.int64)).to("cuda:0")
    d_hk = torch.from_numpy(hk2.view(np.int64)).to("cuda:0")
    d_out = torch.full((20, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    d_diff = torch.full((12, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.gcm_transcipher_device(gpu_context, 128, d_rk.data_ptr(), d_hk.data_ptr(), 4, [(R.IV3, aad, data)], 12, 2,
                             d_out.data_ptr(), d_diff.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), plain)
    assert np.array_equal(d_diff.cpu().numpy().view(np.uint64), diff)


@pytest.fixture(scope="module")
def ragged(gpu_context, rk2, hk2):
    """One call of two frames under the 4-power table at tag_len = 8: m = 1 (nothing hashed but the length block) and
    m = 2 (9 ciphertext bytes and the tag: 17 data bytes, a ragged block).  E(J0) of frame f is source
    (n_powers + f) * 128 + r of the call's plan, behind the whole table and not behind max m = 2 blocks of it."""
    shapes = [(R.IV3, b"", b""), (R.IV3[::-1], b"", bytes((7 * i + 3) & 255 for i in range(9)))]
    frames = [(iv, aad, aes_var.gcm_encrypt_plain(R.KEY3, iv, aad, pt, 8, rounds=2)) for iv, aad, pt in shapes]
    assert [len(R.hashed_blocks(aad, d[:-8])) for _, aad, d in frames] == [1, 2] and len(frames[1][2]) == 17
    return frames, V.gcm_transcipher_raw(gpu_context, rk2, hk2, frames, 8, rounds=2)


def _device_call(torch, ctx, rk, hk, frames, tag_len, n_bytes):
    """gcm_transcipher_device on uploads of rk and hk: the payload bits, the differences and hk read back."""
    d_rk = torch.from_numpy(rk.view(np.int64)).to("cuda:0")
    d_hk = torch.from_numpy(np.ascontiguousarray(hk).view(np.int64)).to("cuda:0")
    d_out = torch.full((n_bytes, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    d_diff = torch.full((len(frames), tag_len, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    V.gcm_transcipher_device(ctx, 128, d_rk.data_ptr(), d_hk.data_ptr(), hk.shape[0], frames, tag_len, 2,
                             d_out.data_ptr(), d_diff.data_ptr())
    return [d.cpu().numpy().view(np.uint64) for d in (d_out, d_diff, d_hk)]


def test_ragged_batch_equals_composition(gpu_context, client, lut_id, rk2, hk2, ragged):
    torch = pytest.importorskip("torch")
    frames, got = ragged
    assert [g[0].shape[0] for g in got] == [0, 9]
    for (iv, aad, data), (plain, diff) in zip(frames, got):
        want_plain, want_diff = _frame_np(gpu_context, lut_id, rk2, hk2, iv, aad, data, 8, 2)
        assert np.array_equal(plain, want_plain)
        assert np.array_equal(diff, want_diff)
        assert aes_var.gcm_tag_ok(client, diff)
    d_plain, d_diff, _ = _device_call(torch, gpu_context, rk2, hk2, frames, 8, 9)
    assert np.array_equal(d_plain, np.concatenate([g[0] for g in got]))
    assert np.array_equal(d_diff, np.stack([g[1] for g in got]))


def test_table_is_read_in_place(gpu_context, rk2, hk2, ragged):
    """Blocks 2..3 of the table lie beyond max m = 2: nothing the result depends on reads them.  The caller's device
    table is a source where it lies and is never written."""
    torch = pytest.importorskip("torch")
    frames, got = ragged
    scribbled = hk2.copy()
    scribbled[2:] = (np.arange(scribbled[2:].size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(scribbled[2:].shape)
    again = V.gcm_transcipher_raw(gpu_context, rk2, scribbled, frames, 8, rounds=2)
    for (plain, diff), (want_plain, want_diff) in zip(again, got):
        assert np.array_equal(plain, want_plain) and np.array_equal(diff, want_diff)
    d_plain, d_diff, hk_after = _device_call(torch, gpu_context, rk2, scribbled, frames, 8, 9)
    assert np.array_equal(d_plain, np.concatenate([g[0] for g in got]))
    assert np.array_equal(d_diff, np.stack([g[1] for g in got]))
    assert np.array_equal(hk_after, scribbled)


def test_chunked_pass_gives_the_same_words(gpu_context, product_raw, rk2, hk2, monkeypatch):
    """The frame of test_single_frame_equals_composition with its three public blocks in chunks of 2: J0 and the first
    counter fall in one chunk, the last counter in the next.  The chunk size is read when the context is created."""
    aad, msg = bytes(range(8)), bytes((13 * i + 7) & 255 for i in range(20))
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, aad, msg, 12, rounds=2)
    (want_plain, want_diff), = V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(R.IV3, aad, data)], 12, rounds=2)
    monkeypatch.setenv("TAE_CTR_CHUNK_BLOCKS", "2")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_CTR_CHUNK_BLOCKS")
    (plain, diff), = V.gcm_transcipher_raw(ctx2, rk2, hk2, [(R.IV3, aad, data)], 12, rounds=2)
    assert np.array_equal(plain, want_plain) and np.array_equal(diff, want_diff)
    del ctx2


def test_ragged_batch_equals_single_frames(gpu_context, client, rk2, hk2):
    iv_b = bytes(range(0x20, 0x2C))
    shapes = [(R.IV3, b"", b""), (iv_b, bytes(range(15)), b""), (R.IV3[::-1], b"", bytes((7 * i + 3) & 255 for i in range(17)))]
    frames = [(iv, aad, aes_var.gcm_encrypt_plain(R.KEY3, iv, aad, pt, 8, rounds=2)) for iv, aad, pt in shapes]
    got = V.gcm_transcipher_raw(gpu_context, rk2, hk2, frames, 8, rounds=2)
    assert [g[0].shape[0] for g in got] == [0, 0, 17]
    for frame, (plain, diff), (_, _, pt) in zip(frames, got, shapes):
        (one_plain, one_diff), = V.gcm_transcipher_raw(gpu_context, rk2, hk2, [frame], 8, rounds=2)
        assert np.array_equal(plain, one_plain)
        assert np.array_equal(diff, one_diff)
        assert _bytes_of(client, plain) == pt and aes_var.gcm_tag_ok(client, diff)


def test_case_4_full_rounds(gpu_context, client, full):
    rk, hk = full
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, R.AAD4, R.PT3[:60])
    assert data[-16:] == R.TAG4
    bad_tag, bad_ct = bytearray(data), bytearray(data)
    bad_tag[-3] ^= 0x10
    bad_ct[5] ^= 0x10
    frames = [(R.IV3, R.AAD4, data), (R.IV3, R.AAD4, bytes(bad_tag)), (R.IV3, R.AAD4, bytes(bad_ct))]
    got = V.gcm_transcipher_raw(gpu_context, rk, hk, frames, 16)
    assert _bytes_of(client, got[0][0]) == R.PT3[:60]
    assert _bytes_of(client, got[0][1]) == bytes(16) and aes_var.gcm_tag_ok(client, got[0][1])
    for (iv, aad, d), (plain, diff) in zip(frames[1:], got[1:]):
        want_plain, want_diff = aes_var.gcm_decrypt_plain(R.KEY3, iv, aad, d)
        assert any(want_diff)
        assert _bytes_of(client, plain) == want_plain
        assert _bytes_of(client, diff) == want_diff and not aes_var.gcm_tag_ok(client, diff)


def test_case_1_j0_only_rows(gpu_context, client):
    """Zero key, zero IV, nothing hashed but the all-zero length block: every row is its E(J0) bit alone."""
    rk = V.key_schedule_raw(gpu_context, client.encrypt_bits_raw(_bits(R.KEY1), start_index=9_050_000))
    hk = V.ghash_key_raw(gpu_context, rk, 1)
    assert _bytes_of(client, hk[0]) == R.H1
    tag = bytes.fromhex("58e2fccefa7e3061367f1d57a4e7455a")
    (plain, diff), = V.gcm_transcipher_raw(gpu_context, rk, hk, [(bytes(12), b"", tag)], 16)
    assert plain.shape[0] == 0 and _bytes_of(client, diff) == bytes(16)


def test_aes256_frame_fourteen_rounds(gpu_context, client):
    rk = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(KEY256))), start_index=9_060_000)
    hk = V.ghash_key_raw(gpu_context, rk, 3)
    iv, aad, msg = bytes(range(0x40, 0x4C)), bytes(range(5)), bytes((19 * i + 2) & 255 for i in range(9))
    data = aes_var.gcm_encrypt_plain(KEY256, iv, aad, msg, 13)
    (plain, diff), = V.gcm_transcipher_raw(gpu_context, rk, hk, [(iv, aad, data)], 13)
    assert diff.shape == (13, 8, BIG)
    assert _bytes_of(client, plain) == msg and aes_var.gcm_tag_ok(client, diff)


def test_bitct_frame_packed(gpu_context, client, rk2):
    """Handles: table bits at level 1, payload bits at 9, a tag-difference bit at its chunk count; the legal XORs;
    both results through FheContext.pack."""
    ek = [gpu_context.bit_from_data(rk2[i], 1) for i in range(44 * W)]
    hk = V.ghash_key(gpu_context, ek, 3)
    assert len(hk) == 3 * 128 and {b.noise_level_squared for b in hk} == {1}
    aad, msg = bytes(range(16)), bytes((23 * i + 4) & 255 for i in range(5))  # m = 3: about 192 sources a row
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, aad, msg, 4)
    (bits, diff), = V.gcm_transcipher(gpu_context, ek, hk, [(R.IV3, aad, data)], 4)
    assert len(bits) == 5 and len(diff) == 4
    assert {b.noise_level_squared for byte in bits for b in byte} == {9}
    _, chunks = aes_var.gcm_tag_rows(R.IV3, aad, data[:-4], 4, 3)
    assert [b.noise_level_squared for byte in diff for b in byte] == [len(R.row_chunks(r)) for r in R.tag_rows(aad, data[:-4], 4)]
    assert [b.noise_level_squared for byte in diff for b in byte] == list(chunks) and max(chunks) > 1
    x = diff[0][0].clone()
    x ^= diff[0][1]
    x ^= bits[1][0]
    assert x.noise_level_squared == int(chunks[0]) + int(chunks[1]) + 9
    packed = gpu_context.pack(bits)
    assert aes_128.decrypt_byte_array_packed(client, packed) == msg
    assert aes_var.gcm_tag_ok(client, gpu_context.pack(diff)) and aes_var.gcm_tag_ok(client, diff)


def test_refusals_leave_the_stage_times(gpu_context, gpu_context8, rk2, hk2):
    tag = bytes(16)
    gpu_context.set_timing(True)
    try:
        V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(R.IV3, b"", tag)], 16, rounds=2)
        before = gpu_context.last_stage_times()
        assert before["pbs_launches"] > 0
        for call in (lambda: V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(bytes(16), b"", tag)], 16),
                     lambda: V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(R.IV3, b"", tag)], 5),
                     lambda: V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(R.IV3, b"", tag[:7])], 8),
                     lambda: V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(R.IV3, b"", tag)], 16, rounds=1),
                     lambda: V.gcm_transcipher_raw(gpu_context, rk2, hk2, [(R.IV3, bytes(64), tag)], 16),  # m = 5 > 4
                     lambda: V.ghash_key_raw(gpu_context, rk2, 0), lambda: V.ghash_key_raw(gpu_context, rk2, 65)):
            assert _code(call) == N.TAE_E_PARAM
        # 100 dense hashed blocks: about 6400 sources a row, 100 chunks.  The table's words are never read: the
        # refusal comes first
        big_hk = np.zeros((128, 128, BIG), dtype=np.uint64)
        long_frame = (R.IV3, b"", bytes([0xA5]) * (99 * 16) + tag)
        assert _code(lambda: V.gcm_transcipher_raw(gpu_context, rk2, big_hk, [long_frame], 16)) == N.TAE_E_NOISE
        assert gpu_context.last_stage_times() == before
    finally:
        gpu_context.set_timing(False)
    k8 = np.zeros((44 * W, gpu_context8.lwe_size), dtype=np.uint64)
    h8 = np.zeros((1, 128, gpu_context8.lwe_size), dtype=np.uint64)
    assert _code(lambda: V.ghash_key_raw(gpu_context8, k8, 1)) == N.TAE_E_PARAM
    assert _code(lambda: V.gcm_transcipher_raw(gpu_context8, k8, h8, [(R.IV3, b"", tag)], 16)) == N.TAE_E_PARAM
