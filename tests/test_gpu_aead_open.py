"""The AEAD open on the GPU (tae_aead_verdict_raw, tae_aead_open_raw, tae_aead_open; the reference has
no AEAD): a verdict bit per frame from its tag-difference bits, and the payload gated by it.

Word-for-word anchors.  The inputs are client-encrypted bits, so no cipher runs except in the end-to-end tests.  The
engine keyswitches every ciphertext once and gathers small ciphertexts into the groups; here the groups are gathered in
numpy from the big ciphertexts, padded with zero ciphertexts, and go through the public circuit_bootstrap_raw with
tables made by generate_lookup_table: the two must give the same words.  Encryption indices 13 000 000 ... are used by
no other test.

The measured-noise tests follow tests/test_gpu_noise.py: the phase error of a last-level verdict bit (level 8) and of
the gate's outputs (a 9-input bootstrap, level 9) against the margin of the next bootstrap, bounds from
tests/noise_ref.py.  noise_ref.margin_floor(m) lowers an estimate from m independent samples by 5 / sqrt(2 m), which
leaves nothing at the three frames of the parity tests, so one call of 256 one-byte frames at tag_len 4 supplies the
samples: m = 256 frames for the verdicts, 256 byte groups for the 2048 gated bits.
Each point prints (run with -s):  noise: name level m log2(std_big) log2(std_small) margin margin*floor/z_required
"""
import math

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var
from tests import gcm_ref as G
from tests import noise_ref as R

pytestmark = pytest.mark.gpu

BIG = 4 * 512 + 1
V = aes_var.GalMulAes
W = 32
LENS = (17, 0, 3)
AT = 13_000_000
CCM_KEY = bytes(range(0x40, 0x50))


def _bits(data):
    return [b for byte in data for b in aes_128.u8_to_bits(byte)]


def _bytes_of(client, cts):
    bits = client.decrypt_bits_raw(cts.reshape(-1, cts.shape[-1])).reshape(-1, 8)
    return bytes(aes_128.bits_to_u8(b) for b in bits)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


def f_or8(v):
    return int(v != 0)


def f_nor8(v):
    return int(v == 0)


def f_gate(v):
    """v = the byte's 8 bits, then the verdict: the byte where the verdict is 1."""
    return (v >> 1) if v & 1 else 0


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.fixture(scope="module")
def luts(gpu_context):
    g = gpu_context.generate_lookup_table
    return g(8, 1, f_or8), g(8, 1, f_nor8), g(9, 8, f_gate)


def _diffs(client, tag_len, ones, start):
    """[n][8 tag_len][BIG] fresh encryptions of difference bits: frame f all zero but a 1 at ones[f] (None: authentic)."""
    bits = np.zeros((len(ones), 8 * tag_len), dtype=np.uint8)
    for f, at in enumerate(ones):
        if at is not None:
            bits[f, at] = 1
    return client.encrypt_bits_raw(bits.ravel(), start_index=start).reshape(len(ones), 8 * tag_len, BIG)


def _verdict_np(ctx, luts, diff):
    """The public path: every level's groups gathered from big ciphertexts and zero-padded."""
    cur = diff
    while True:
        n, bits = cur.shape[:2]
        groups = -(-bits // 8)
        padded = np.zeros((n, groups * 8, BIG), dtype=np.uint64)
        padded[:, :bits] = cur
        last = groups == 1
        out = ctx.circuit_bootstrap_raw(padded.reshape(n * groups, 8, BIG), luts[1] if last else luts[0])
        cur = out.reshape(n, groups, BIG)
        if last:
            return cur[:, 0]


def _gate_np(ctx, luts, plain, ok):
    """plain: per frame [len][8][BIG]; ok [n][BIG] -> per frame the 9 -> 8 bootstrap of (byte, the frame's verdict)."""
    groups = [np.concatenate([byte, ok[f][None]]) for f, frame in enumerate(plain) for byte in frame]
    out = ctx.circuit_bootstrap_raw(np.stack(groups), luts[2])
    res, at = [], 0
    for frame in plain:
        res.append(out[at:at + len(frame)])
        at += len(frame)
    return res


@pytest.fixture(scope="module")
def three(client):
    """Three frames at tag_len 13 (104 -> 13 -> 2 -> 1, ragged at two levels): authentic, a 1 in the last difference bit,
    a 1 in bit 0; payloads of 17, 0 and 3 bytes."""
    msgs = [bytes((29 * i + 11 * f + 5) & 255 for i in range(n)) for f, n in enumerate(LENS)]
    plain = [client.encrypt_bits_raw(_bits(m), start_index=AT + 1000 * f).reshape(len(m), 8, BIG) if m
             else np.zeros((0, 8, BIG), dtype=np.uint64) for f, m in enumerate(msgs)]
    return msgs, plain, _diffs(client, 13, (None, 103, 0), AT + 10_000)


@pytest.fixture(scope="module")
def opened(gpu_context, three):
    """The three-frame open on the session's context: (per frame the gated payload, ok [3][BIG])."""
    _, plain, diff = three
    return aes_var.aead_open_raw(gpu_context, plain, diff, 13)


# ---- the verdict ----------------------------------------------------------------------------------------------------
def test_verdict_equals_public_composition(gpu_context, client, luts, three):
    _, _, diff = three
    ok = aes_var.aead_verdict_raw(gpu_context, diff, 13)
    assert ok.shape == (3, BIG)
    assert np.array_equal(ok, _verdict_np(gpu_context, luts, diff))
    assert list(client.decrypt_bits_raw(ok)) == [1, 0, 0]
    assert [aes_var.open_ok(client, o) for o in ok] == [True, False, False]


def test_verdict_two_levels(gpu_context, client, luts):
    diff = _diffs(client, 4, (None, 31, 0), AT + 20_000)
    ok = aes_var.aead_verdict_raw(gpu_context, diff, 4)
    assert np.array_equal(ok, _verdict_np(gpu_context, luts, diff))
    assert list(client.decrypt_bits_raw(ok)) == [1, 0, 0]


# ---- the gate -------------------------------------------------------------------------------------------------------
def test_gate_equals_public_composition(gpu_context, client, luts, three, opened):
    torch = pytest.importorskip("torch")
    msgs, plain, diff = three
    got, ok = opened
    assert [g.shape for g in got] == [(n, 8, BIG) for n in LENS] and ok.shape == (3, BIG)
    assert np.array_equal(ok, aes_var.aead_verdict_raw(gpu_context, diff, 13))
    want = _gate_np(gpu_context, luts, plain, ok)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert _bytes_of(client, got[0]) == msgs[0] and _bytes_of(client, got[2]) == bytes(3)
    # device memory: the same words, nothing staged
    flat = np.concatenate(plain)
    d_plain = torch.from_numpy(flat.view(np.int64)).to("cuda:0")
    d_diff = torch.from_numpy(diff.view(np.int64)).to("cuda:0")
    d_out = torch.full(flat.shape, -1, dtype=torch.int64, device="cuda:0")
    d_ok = torch.full((3, BIG), -1, dtype=torch.int64, device="cuda:0")
    aes_var.aead_open_device(gpu_context, d_plain.data_ptr(), LENS, d_diff.data_ptr(), 13, d_out.data_ptr(), d_ok.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), np.concatenate(got))
    assert np.array_equal(d_ok.cpu().numpy().view(np.uint64), ok)


def test_chunked_pass_gives_the_same_words(product_raw, three, opened, monkeypatch):
    """With one block per chunk a gate pass is 14 bytes: the 17-byte frame crosses the pass boundary and the verdict index
    changes inside pass 2.  The chunk size is read when the context is created."""
    _, plain, diff = three
    monkeypatch.setenv("TAE_CTR_CHUNK_BLOCKS", "1")
    ctx2 = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    monkeypatch.delenv("TAE_CTR_CHUNK_BLOCKS")
    got, ok = aes_var.aead_open_raw(ctx2, plain, diff, 13)
    del ctx2
    assert np.array_equal(ok, opened[1])
    for g, w in zip(got, opened[0]):
        assert np.array_equal(g, w)


def test_batch_equals_single_frames(gpu_context, three, opened):
    _, plain, diff = three
    for f in (1, 0):  # the frame without payload, then the one that keeps its payload
        got, ok = aes_var.aead_open_raw(gpu_context, [plain[f]], diff[f:f + 1], 13)
        assert np.array_equal(ok[0], opened[1][f]) and np.array_equal(got[0], opened[0][f])


# ---- call order -----------------------------------------------------------------------------------------------------
def test_first_call_and_after_other_calls(gpu_context, client, product_raw, three, opened):
    """The open shares d_small_, the GCM scratch and the circuit bootstrap's buffers: its words as the first compute
    call of a fresh context equal its words after a two-round GCM call and after a circuit bootstrap with another
    table."""
    _, plain, diff = three

    def same(res):
        return np.array_equal(res[1], opened[1]) and all(np.array_equal(g, w) for g, w in zip(res[0], opened[0]))

    ctx = tfhe_aes.context_from_raw(tfhe_aes.PARAMS_SQRD_LVL_64, product_raw[1], device=0)
    assert same(aes_var.aead_open_raw(ctx, plain, diff, 13))
    rk = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(G.KEY3))), start_index=AT + 30_000)
    hk = V.ghash_key_raw(ctx, rk, 2, rounds=2)
    data = aes_var.gcm_encrypt_plain(G.KEY3, G.IV3, b"", bytes(range(5)), 12, rounds=2)
    V.gcm_transcipher_raw(ctx, rk, hk, [(G.IV3, b"", data)], 12, rounds=2)
    assert same(aes_var.aead_open_raw(ctx, plain, diff, 13))
    other = ctx.generate_lookup_table(8, 24, lambda x: (aes_128.SBOX[x] << 16) | x)
    ctx.circuit_bootstrap_raw(plain[0][:5], other)
    assert same(aes_var.aead_open_raw(ctx, plain, diff, 13))
    del ctx


# ---- end to end -----------------------------------------------------------------------------------------------------
def _handles(ctx, client, key, start):
    rk = client.encrypt_bits_raw(_bits(b"".join(aes_var.key_schedule_plain(key))), start_index=start)
    return [ctx.bit_from_data(rk[i], 1) for i in range(44 * W)]


def test_gcm_open_full_rounds(gpu_context, client):
    """8 bytes of AAD and 20 of payload (m = 4, n_powers = 4) at ten rounds, authentic and with one ciphertext bit
    flipped, through the handle form: levels 9 and 8, and the result through FheContext.pack."""
    ek = _handles(gpu_context, client, G.KEY3, AT + 40_000)
    hk = V.ghash_key(gpu_context, ek, 4)
    aad, msg = bytes(range(8)), bytes((13 * i + 7) & 255 for i in range(20))
    data = aes_var.gcm_encrypt_plain(G.KEY3, G.IV3, aad, msg, 16)
    bad = bytearray(data)
    bad[5] ^= 0x10
    plain, ok = V.gcm_open(gpu_context, ek, hk, [(G.IV3, aad, data), (G.IV3, aad, bytes(bad))], 16)
    assert [len(p) for p in plain] == [20, 20] and len(ok) == 2
    assert {b.noise_level_squared for frame in plain for byte in frame for b in byte} == {9}
    assert [o.noise_level_squared for o in ok] == [8, 8]
    assert [aes_var.open_ok(client, o) for o in ok] == [True, False]
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(plain[0])) == msg
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(plain[1])) == bytes(20)
    # fresh ids: a gated bit adds to a verdict and to another gated bit
    x = plain[0][0][0].clone()
    x ^= plain[0][0][1]
    x ^= ok[0]
    assert x.noise_level_squared == 9 + 9 + 8


def test_ccm_open_two_rounds(gpu_context, client):
    ek = _handles(gpu_context, client, CCM_KEY, AT + 50_000)
    nonce, aad, msg = bytes(range(0x10, 0x1D)), bytes(range(6)), bytes((17 * i + 3) & 255 for i in range(9))
    data = aes_var.ccm_encrypt_plain(CCM_KEY, nonce, aad, msg, 8, rounds=2)
    bad = bytearray(data)
    bad[-2] ^= 0x01
    for frame in (data, bytes(bad)):
        want_plain, want_diff = aes_var.ccm_decrypt_plain(CCM_KEY, nonce, aad, frame, 8, rounds=2)
        authentic = not any(want_diff)
        bits, ok = V.ccm_open(gpu_context, ek, nonce, aad, frame, 8, rounds=2)
        assert aes_var.open_ok(client, ok) == authentic and ok.noise_level_squared == 8
        got = bytes(aes_128.bits_to_u8([client.decrypt(b).value for b in byte]) for byte in bits)
        assert got == (want_plain if authentic else bytes(9))
    assert authentic is False


def test_multi_key_ccm_open_and_gcm_long_open_two_rounds(gpu_context, client):
    """The other two conveniences: frames under two keys of a table, and a frame of two GHASH segments."""
    from tfhe_aes import aes_multi
    keys = [CCM_KEY, bytes(range(0x70, 0x80))]
    table = [_handles(gpu_context, client, k, AT + 60_000 + 2000 * s) for s, k in enumerate(keys)]
    nonce, aad = bytes(range(0x30, 0x37)), bytes(range(3))
    msgs = [bytes((5 * i + 1) & 255 for i in range(4)), bytes((9 * i + 2) & 255 for i in range(6))]
    data = [aes_var.ccm_encrypt_plain(keys[s], nonce, aad, msgs[s], 4, rounds=2) for s in (0, 1)]
    forged = bytes([data[1][0] ^ 0x80]) + data[1][1:]
    plain, ok = aes_multi.GalMulAesMulti.ccm_open(gpu_context, table, [(1, nonce, aad, forged), (0, nonce, aad, data[0])], 4,
                                                  rounds=2)
    assert [aes_var.open_ok(client, o) for o in ok] == [False, True]
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(plain[0])) == bytes(6)
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(plain[1])) == msgs[0]
    # 8 bytes of AAD and 20 of payload hash m = 4 blocks: two segments of seg = 2, one stride power
    ek = table[0]
    hk = V.ghash_key(gpu_context, ek, 2, rounds=2)
    sk = V.ghash_stride_key(gpu_context, hk, 2, 1)
    msg = bytes((13 * i + 7) & 255 for i in range(20))
    frame = aes_var.gcm_encrypt_plain(CCM_KEY, G.IV3, bytes(range(8)), msg, 12, rounds=2)
    plain, ok = V.gcm_long_open(gpu_context, ek, hk, sk, 2, [(G.IV3, bytes(range(8)), frame)], 12, rounds=2)
    assert aes_var.open_ok(client, ok[0]) and ok[0].noise_level_squared == 8
    assert aes_128.decrypt_byte_array_packed(client, gpu_context.pack(plain[0])) == msg


# ---- measured noise -------------------------------------------------------------------------------------------------
N_SAMPLES = 256


@pytest.fixture(scope="module")
def sample(gpu_context, client):
    """256 one-byte frames at tag_len 4: every other frame authentic, the rest with a 1 at a random difference bit."""
    rng = np.random.default_rng(131)
    ones = [None if f % 2 == 0 else int(rng.integers(0, 32)) for f in range(N_SAMPLES)]
    diff = _diffs(client, 4, ones, AT + 100_000)
    data = rng.integers(0, 256, N_SAMPLES)
    plain = client.encrypt_bits_raw(_bits(data), start_index=AT + 200_000).reshape(N_SAMPLES, 1, 8, BIG)
    got, ok = aes_var.aead_open_raw(gpu_context, list(plain), diff, 4)
    ok_bits = np.array([1 if o is None else 0 for o in ones], dtype=np.uint8)
    out_bits = np.array([_bits([int(d) if k else 0]) for d, k in zip(data, ok_bits)], dtype=np.uint8)
    return ok, ok_bits, np.concatenate(got), out_bits


def _point(ctx, client, name, level, m, cts, bits):
    from tests.test_gpu_noise import _errors
    eb, es = _errors(ctx, client, cts, bits)
    margin = R.margin(es, client)
    print("noise: %-28s %-3d %5d %6.2f %6.2f %6.2f %6.3f" % (name, level, m, math.log2(eb.std()), math.log2(es.std()),
                                                            margin, margin * R.margin_floor(m) / R.z_required()))
    assert np.abs(es).max() < R.HALF_GAP and np.abs(eb).max() < R.HALF_GAP, (name, "a sample beyond 2^62")
    assert margin * R.margin_floor(m) >= R.z_required(), (name, "margin", margin, m)


def test_measured_noise_of_a_verdict_bit(gpu_context, client, sample):
    print()
    ok, ok_bits, _, _ = sample
    assert np.array_equal(client.decrypt_bits_raw(ok), ok_bits)
    _point(gpu_context, client, "verdict bit (last level)", 8, N_SAMPLES, ok, ok_bits)


def test_measured_noise_of_the_gated_payload(gpu_context, client, sample):
    print()
    _, _, out, out_bits = sample
    assert np.array_equal(client.decrypt_bits_raw(out.reshape(-1, BIG)), out_bits.ravel())
    _point(gpu_context, client, "gated payload bit (9 -> 8)", 9, N_SAMPLES, out, out_bits)


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stage_times(gpu_context, gpu_context8, three):
    _, plain, diff = three
    gpu_context.set_timing(True)
    try:
        aes_var.aead_verdict_raw(gpu_context, diff[:1], 13)
        before = gpu_context.last_stage_times()
        # 104 -> 13 -> 2 -> 1: three levels of cbs_l = 1 launches; the keyswitches and the gathers are timed
        assert before["pbs_launches"] == 3 and before["keyswitch"] > 0 and before["linear"] > 0
        flat = np.concatenate(plain)
        for tag_len in (0, 5, 11, 17):
            wrong = np.zeros((1, max(8 * tag_len, 1), BIG), dtype=np.uint64)
            ok = np.zeros((1, BIG), dtype=np.uint64)
            assert N.lib().tae_aead_verdict_raw(gpu_context._h, wrong.ctypes.data, 1, tag_len, ok.ctypes.data,
                                                N.TAE_MEM_HOST) == N.TAE_E_PARAM
        lens = np.array(LENS, dtype=np.uintp)
        assert N.lib().tae_aead_open_raw(gpu_context._h, flat.ctypes.data, lens.ctypes.data, diff.ctypes.data, 3, 9,
                                         flat.ctypes.data, diff.ctypes.data, N.TAE_MEM_HOST) == N.TAE_E_PARAM
        assert N.lib().tae_aead_open_raw(gpu_context._h, None, lens.ctypes.data, diff.ctypes.data, 3, 13,
                                         flat.ctypes.data, diff.ctypes.data, N.TAE_MEM_HOST) == N.TAE_E_ARG
        # no frames: nothing runs
        assert aes_var.aead_verdict_raw(gpu_context, np.zeros((0, 104, BIG), dtype=np.uint64), 13).shape == (0, BIG)
        # the handle form on an input above the cap
        loud = [gpu_context.bit_from_data(diff[0, i], 65 if i == 7 else 1) for i in range(104)]
        assert _code(lambda: aes_var.aead_open(gpu_context, [], [loud], [0], 13)) == N.TAE_E_NOISE
        assert gpu_context.last_stage_times() == before
    finally:
        gpu_context.set_timing(False)
    d8 = np.zeros((1, 32, gpu_context8.lwe_size), dtype=np.uint64)
    assert _code(lambda: aes_var.aead_verdict_raw(gpu_context8, d8, 4)) == N.TAE_E_PARAM
    p8 = np.zeros((1, 8, gpu_context8.lwe_size), dtype=np.uint64)
    assert _code(lambda: aes_var.aead_open_raw(gpu_context8, [p8], d8, 4)) == N.TAE_E_PARAM
