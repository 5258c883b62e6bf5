"""AES-GCM over key tables on the GPU (tae_aesm_ghash_key*, tae_aesm_gcm_transcipher*).

The contract of every multi-key entry point: slot s of the power tables, and every frame's words, equal what the
single-key call gives on that slot's key and table, word for word.  Where words are compared the cipher runs 2 rounds;
full rounds are checked through decryption against the GCM specification's test cases 2 and 4.
"""
import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_multi, aes_var
from tests import gcm_ref as R

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
V = aes_var.GalMulAes
M = aes_multi.GalMulAesMulti
W = 32
KEYS = (bytes(range(0x10, 0x20)), R.KEY3, bytes((7 * i + 3) & 255 for i in range(16)))
AT = 12_000_000
TAG2 = bytes.fromhex("ab6e47d42cec13bdf53a67b21257bddf")  # test case 2
CT2 = bytes.fromhex("0388dace60b6a392f328c2b971b2fe78")


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _bytes_of(client, cts):
    bits = client.decrypt_bits_raw(cts.reshape(-1, cts.shape[-1])).reshape(-1, 8)
    return bytes(aes_128.bits_to_u8(b) for b in bits)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
                                         for g, w in zip(got, want))


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def table(client):
    """Three 128-bit slots: fresh encryptions of plain expanded keys."""
    return np.stack([client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(k))), start_index=AT + 10_000 * s)
                     for s, k in enumerate(KEYS)])


@pytest.fixture(scope="module")
def htable(gpu_context, table):
    """n_powers = 4 at 2 rounds: one product (the power 3) and the squares for 2 and 4, per slot."""
    return M.ghash_key_raw(gpu_context, table, 4, rounds=2)


def _frames4():
    """Slots [2, 0, 2, 0], tag_len 12: an empty frame (m = 1), 15 bytes of AAD alone, 17 bytes of payload alone, 8 bytes
    of AAD with 20 of payload (m = 4)."""
    iv_b = bytes(range(0x20, 0x2C))
    shapes = [(2, R.IV3, b"", b""), (0, iv_b, bytes(range(15)), b""),
              (2, R.IV3[::-1], b"", bytes((7 * i + 3) & 255 for i in range(17))),
              (0, R.IV3, bytes(range(8)), bytes((13 * i + 7) & 255 for i in range(20)))]
    frames = [(s, iv, aad, aes_var.gcm_encrypt_plain(KEYS[s], iv, aad, pt, 12, rounds=2)) for s, iv, aad, pt in shapes]
    return shapes, frames


@pytest.fixture(scope="module")
def got4(gpu_context, table, htable):
    return M.gcm_transcipher_raw(gpu_context, table, htable, _frames4()[1], 12, rounds=2)


def _device_call(torch, ctx, table, htable, frames, tag_len, total):
    """The device-memory variant into sentinel-filled buffers -> (plain [total][8][BIG], diff [n][tag_len][8][BIG])."""
    d_tab = torch.from_numpy(table.view(np.int64)).to("cuda:0")
    d_htab = torch.from_numpy(np.ascontiguousarray(htable).view(np.int64)).to("cuda:0")
    d_out = torch.full((max(total, 1), 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    d_diff = torch.full((len(frames), tag_len, 8, BIG), -1, dtype=torch.int64, device="cuda:0")
    M.gcm_transcipher_device(ctx, 128, d_tab.data_ptr(), table.shape[0], d_htab.data_ptr(), htable.shape[1], frames,
                             tag_len, 2, d_out.data_ptr(), d_diff.data_ptr())
    return d_out.cpu().numpy().view(np.uint64)[:total], d_diff.cpu().numpy().view(np.uint64)


# ---- 1. the power tables --------------------------------------------------------------------------------------------
def test_table_equals_single_key_tables(gpu_context, client, table, htable):
    torch = pytest.importorskip("torch")
    assert htable.shape == (3, 4, 128, BIG)
    for s in range(3):
        assert np.array_equal(htable[s], V.ghash_key_raw(gpu_context, table[s], 4, rounds=2))
    d_tab = torch.from_numpy(table.view(np.int64)).to("cuda:0")
    d_out = torch.full((3, 4, 128, BIG), -1, dtype=torch.int64, device="cuda:0")
    M.ghash_key_device(gpu_context, 128, d_tab.data_ptr(), 3, 4, 2, d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), htable)
    # a table is H, H^2, H^3, H^4 of whatever H the two-round cipher gives
    for s in range(3):
        p = [_bytes_of(client, t) for t in htable[s]]
        assert p[1] == R.mul(p[0], p[0]) and p[2] == R.mul(p[1], p[0]) and p[3] == R.mul(p[1], p[1])


# ---- 2. where a product batch ends changes nothing ------------------------------------------------------------------
def test_product_batching_changes_nothing(product_raw, table, htable, monkeypatch):
    """With one product per batch the batch boundary of generation 2 falls between the slots.  The batch size is read
    when the context is created."""
    monkeypatch.setenv("TAE_GCM_SEG_BATCH", "1")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_GCM_SEG_BATCH")
    assert np.array_equal(M.ghash_key_raw(ctx2, table, 4, rounds=2), htable)
    del ctx2


# ---- 3. frames ------------------------------------------------------------------------------------------------------
def test_frames_equal_single_key_calls(gpu_context, client, table, htable, got4):
    torch = pytest.importorskip("torch")
    shapes, frames = _frames4()
    assert [g[0].shape for g in got4] == [(n, 8, BIG) for n in (0, 0, 17, 20)]
    assert all(g[1].shape == (12, 8, BIG) for g in got4)
    for (s, iv, aad, data), (_, _, _, pt), (plain, diff) in zip(frames, shapes, got4):
        (one_plain, one_diff), = V.gcm_transcipher_raw(gpu_context, table[s], htable[s], [(iv, aad, data)], 12, rounds=2)
        assert np.array_equal(plain, one_plain)
        assert np.array_equal(diff, one_diff)
        assert _bytes_of(client, plain) == pt and aes_var.gcm_tag_ok(client, diff)
    d_plain, d_diff = _device_call(torch, gpu_context, table, htable, frames, 12, 37)
    assert np.array_equal(d_plain, np.concatenate([g[0] for g in got4]))
    assert np.array_equal(d_diff, np.stack([g[1] for g in got4]))


# ---- 4. a slot no frame names -----------------------------------------------------------------------------------------
def test_unreferenced_slot_is_not_read(gpu_context, table, htable, got4):
    torch = pytest.importorskip("torch")
    _, frames = _frames4()
    rnd = np.random.default_rng(7)
    t2, h2 = table.copy(), htable.copy()
    t2[1] = rnd.integers(0, 1 << 63, size=t2[1].shape, dtype=np.uint64) * np.uint64(3)
    h2[1] = rnd.integers(0, 1 << 63, size=h2[1].shape, dtype=np.uint64) * np.uint64(5)
    assert _same(M.gcm_transcipher_raw(gpu_context, t2, h2, frames, 12, rounds=2), got4)
    d_plain, d_diff = _device_call(torch, gpu_context, t2, h2, frames, 12, 37)
    assert np.array_equal(d_plain, np.concatenate([g[0] for g in got4]))
    assert np.array_equal(d_diff, np.stack([g[1] for g in got4]))


# ---- 5. full rounds against the specification -----------------------------------------------------------------------
def test_full_rounds_against_the_specification(gpu_context, client):
    keys = np.stack([client.encrypt_bits_raw(_bits(k), start_index=AT + 100_000 + 1000 * s)
                     for s, k in enumerate((R.KEY1, R.KEY3))])
    tab = M.key_schedule_raw(gpu_context, keys)
    htab = M.ghash_key_raw(gpu_context, tab, 8)
    want, p = [], aes_var.encrypt_block_plain(aes_var.key_schedule_plain(R.KEY3), bytes(16))
    h = p
    for _ in range(8):
        want.append(p)
        p = R.mul(p, h)
    assert [_bytes_of(client, t) for t in htab[1]] == want
    assert _bytes_of(client, htab[0][0]) == R.H1
    data4 = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, R.AAD4, R.PT3[:60])
    assert data4[-16:] == R.TAG4
    bad = bytearray(data4)
    bad[-3] ^= 0x10
    frames = [(0, bytes(12), b"", CT2 + TAG2), (1, R.IV3, R.AAD4, data4), (1, R.IV3, R.AAD4, bytes(bad))]
    got = M.gcm_transcipher_raw(gpu_context, tab, htab, frames, 16)
    assert _bytes_of(client, got[0][0]) == bytes(16) and _bytes_of(client, got[0][1]) == bytes(16)
    assert _bytes_of(client, got[1][0]) == R.PT3[:60] and _bytes_of(client, got[1][1]) == bytes(16)
    want_plain, want_diff = aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, R.AAD4, bytes(bad))
    assert any(want_diff) and want_plain == R.PT3[:60]
    assert _bytes_of(client, got[2][0]) == want_plain and _bytes_of(client, got[2][1]) == want_diff
    assert [aes_var.gcm_tag_ok(client, g[1]) for g in got] == [True, True, False]


# ---- 6. handles and open --------------------------------------------------------------------------------------------
def test_handles_and_open(gpu_context, client, table):
    """Two slots at 2 rounds, n_powers = 3.  Levels as the single-key call's: table bits at 1, payload bits at 9, a
    difference bit at its chunk count (16 bytes of AAD and 5 of payload: m = 3, more than one chunk a row)."""
    eks = [[gpu_context.bit_from_data(table[s][i], 1) for i in range(44 * W)] for s in (0, 1)]
    hks = M.ghash_key(gpu_context, eks, 3, rounds=2)
    assert [len(t) for t in hks] == [3 * 128] * 2
    assert {b.noise_level_squared for t in hks for b in t} == {1}
    one_hk = V.ghash_key(gpu_context, eks[1], 3, rounds=2)
    assert [b.noise_level_squared for b in one_hk] == [b.noise_level_squared for b in hks[1]]
    aad, msg = bytes(range(16)), bytes((23 * i + 4) & 255 for i in range(5))
    data = [aes_var.gcm_encrypt_plain(KEYS[s], R.IV3, aad, msg, 4, rounds=2) for s in (0, 1)]
    forged = bytes([data[0][0] ^ 0x80]) + data[0][1:]
    streams = [(1, R.IV3, aad, data[1]), (0, R.IV3, aad, forged)]
    res = M.gcm_transcipher(gpu_context, eks, hks, streams, 4, rounds=2)
    (one_bits, one_diff), = V.gcm_transcipher(gpu_context, eks[1], hks[1], [(R.IV3, aad, data[1])], 4, rounds=2)
    bits, diff = res[0]
    assert len(bits) == 5 and len(diff) == 4
    assert {b.noise_level_squared for byte in bits for b in byte} == {9}
    levels = [b.noise_level_squared for byte in diff for b in byte]
    assert levels == [b.noise_level_squared for byte in one_diff for b in byte]
    assert levels == [len(R.row_chunks(r)) for r in R.tag_rows(aad, data[1][:-4], 4)] and max(levels) > 1
    assert [b.noise_level_squared for byte in bits for b in byte] == [b.noise_level_squared for byte in one_bits for b in byte]
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(bits)) == msg
    assert aes_var.gcm_tag_ok(client, gpu_context.pack(diff)) and not aes_var.gcm_tag_ok(client, res[1][1])
    # a slot no frame names may be None in both tables
    res1 = M.gcm_transcipher(gpu_context, [None, eks[1]], [None, hks[1]], streams[:1], 4, rounds=2)
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(res1[0][0])) == msg
    plain, ok = M.gcm_open(gpu_context, eks, hks, streams, 4, rounds=2)
    assert [aes_var.open_ok(client, o) for o in ok] == [True, False]
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(plain[0])) == msg
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(plain[1])) == bytes(5)


# ---- 7. a cold context ----------------------------------------------------------------------------------------------
def test_cold_context_gives_the_warm_words(product_raw, table, htable, got4):
    ctx = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    assert np.array_equal(M.ghash_key_raw(ctx, table, 4, rounds=2), htable)
    del ctx
    ctx = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    assert _same(M.gcm_transcipher_raw(ctx, table, htable, _frames4()[1], 12, rounds=2), got4)
    del ctx


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stage_times(gpu_context, gpu_context8, table, htable):
    tag = bytes(12)
    good = (2, R.IV3, bytes(8), bytes(20) + tag)  # m = 4
    call = lambda streams, t=12, rounds=2, h=htable: M.gcm_transcipher_raw(gpu_context, table, h, streams, t, rounds=rounds)
    gpu_context.set_timing(True)
    try:
        call([(0, R.IV3, b"", tag)])
        before = gpu_context.last_stage_times()
        assert before["pbs_launches"] > 0
        for slot in (3, -1):
            assert _code(lambda: call([good, (slot, R.IV3, b"", tag)])) == N.TAE_E_ARG
        for bad in (lambda: call([good], h=htable[:, :3]),                   # m = 4 > n_powers = 3
                    lambda: call([(0, R.IV3, bytes(17), bytes(20) + tag)]),  # m = 5 > 4
                    lambda: call([good, (1, R.IV3, b"", bytes(8))]),         # a frame of another tag length
                    lambda: call([good], t=5),
                    lambda: call([(0, bytes(16), b"", tag)]),
                    lambda: call([good], rounds=1),
                    lambda: M.ghash_key_raw(gpu_context, table, 0), lambda: M.ghash_key_raw(gpu_context, table, 65),
                    lambda: M.ghash_key_raw(gpu_context, table, 4, rounds=11)):
            assert _code(bad) == N.TAE_E_PARAM
        assert gpu_context.last_stage_times() == before
    finally:
        gpu_context.set_timing(False)
    t8 = np.zeros((2, 44 * W, gpu_context8.lwe_size), dtype=np.uint64)
    h8 = np.zeros((2, 1, 128, gpu_context8.lwe_size), dtype=np.uint64)
    assert _code(lambda: M.ghash_key_raw(gpu_context8, t8, 1)) == N.TAE_E_PARAM
    assert _code(lambda: M.gcm_transcipher_raw(gpu_context8, t8, h8, [(0, R.IV3, b"", bytes(16))], 16)) == N.TAE_E_PARAM
