"""Packed ciphertext I/O on the GPU (include/tfhe_aes_gpu.h "packed ciphertext I/O").

Unpack: the sample extraction of client-made GLWEs, word for word against a numpy restatement of the index map of
glwe_pack.hpp, every extracted bit decrypting, host and device memory alike.

Pack: GLWE g = sum_j X^j PFKS_{q=k}(bit g N + j), word for word against the same sum over the oracle's private
functional keyswitch (Keys.pfks(k, .), threads over the rows), on real PBS outputs (the fixture of
test_gpu_pfks_variants.py: row 0 on the clamp boundary) and on crafted keys and rows (tests/edge_inputs.py: under a
uniform key every column looks alike, a wrong column offset of the key slice, of corr[] or of the clamp fix-up shows
under pattern_key).  Small counts take the row-limb GEMM, 2085 the K layout by itself (a ragged 384-row tile, a
ragged last GLWE of 37 bits); which kernel ran is read from the engine.

End to end: two AES-128 blocks, full rounds, the key uploaded packed and the result returned packed.
"""
import ctypes as C
import os

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128, aes_var
from tests import edge_inputs as E
from tests.packed_ref import BIG, GLWE, PK, PN, U64, extract_np, oracle_pack
from tests.test_gpu_pfks_variants import pbs_outputs  # noqa: F401  (module fixture: real PBS outputs, crafted row 0)

pytestmark = pytest.mark.gpu

B_AUTO = 2048 + 37
VARIANTS = ("g6", "s16", "w32", "w16")
DEFAULT = "w16"
V = aes_var.GalMulAes
PID = tfhe_aes.PARAMS_SQRD_LVL_64


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _context(keys, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return tfhe_aes.context_from_raw(PID, keys, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


def _pack(ctx, rows, want):
    out = ctx.pack(rows)
    assert ctx.last_pfks_kernel() == want
    assert out.origin == "server" and out.count == len(rows) and out.data.shape == ((len(rows) + PN - 1) // PN, GLWE)
    return out.data


# ---- unpack ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 512, 513, 1030))
def test_unpack_equals_the_index_map(gpu_context, client, oracle_keys, count):
    torch = pytest.importorskip("torch")
    bits = np.random.default_rng(count).integers(0, 2, size=count).astype(np.uint8)
    up = client.encrypt_packed(bits, start_index=40_000)
    got = gpu_context.unpack_raw(up)
    assert np.array_equal(got, extract_np(up.data, count))
    assert np.array_equal(client.decrypt_bits_raw(got), bits)
    assert np.array_equal(oracle_keys.decrypt_bits(got), bits)
    d_in = torch.from_numpy(up.data.view(np.int64)).cuda()
    d_out = torch.full((count, BIG), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu_context.unpack_device(d_in.data_ptr(), count, d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(U64), got)


def test_unpack_handles_are_fresh_bits(gpu_context, client):
    bits = [1, 0, 1, 1, 0, 0, 1, 0, 1]
    up = client.encrypt_packed(bits, start_index=41_000)
    hs = gpu_context.unpack(up)
    assert [client.decrypt(h).value for h in hs] == bits
    assert all(h.noise_level_squared == 1 for h in hs)
    hs[0] ^= hs[1]  # distinct ids: the sum is allowed and has noise^2 2
    assert hs[0].noise_level_squared == 2 and client.decrypt(hs[0]).value == 1
    with pytest.raises(ValueError):
        gpu_context.unpack(tfhe_aes.PackedBits(up.data, up.count, "server"))


# ---- pack, real key --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 3, 512, 513))
def test_pack_small_counts_equal_oracle(gpu_context, oracle_keys, pbs_outputs, count):  # noqa: F811
    rows = pbs_outputs[:count]
    got = _pack(gpu_context, rows, "rows")
    for g in range(len(got)):
        assert np.array_equal(got[g], oracle_pack(oracle_keys, rows[g * PN:(g + 1) * PN])), (count, g)


@pytest.fixture(scope="module")
def packed_auto(gpu_context, pbs_outputs):  # noqa: F811
    """B_AUTO bits on the K layout, by itself, on the default kernel."""
    return _pack(gpu_context, pbs_outputs, os.environ.get("TAE_PFKS_GEMM", DEFAULT).split(":")[0])


def test_pack_k_layout_equals_oracle(packed_auto, oracle_keys, pbs_outputs):  # noqa: F811
    """GLWE 0 holds the crafted clamp-boundary row, GLWE 4 is the ragged last one (37 bits, rows 2048.. of the
    ragged sixth 384-row tile)."""
    assert packed_auto.shape == (5, GLWE)
    for g in (0, 4):
        assert np.array_equal(packed_auto[g], oracle_pack(oracle_keys, pbs_outputs[g * PN:(g + 1) * PN])), g


def test_pack_k_layout_equals_row_layout(packed_auto, product_raw, pbs_outputs):  # noqa: F811
    rows_ctx = _context(product_raw[1], {"TAE_PFKS_LAYOUT": "rows"})
    assert np.array_equal(_pack(rows_ctx, pbs_outputs, "rows"), packed_auto)


def test_pack_gemm_variants_agree(product_raw, pbs_outputs):  # noqa: F811
    ref = _pack(_context(product_raw[1], {"TAE_PFKS_GEMM": "w16"}), pbs_outputs, "w16")
    for variant in VARIANTS[:3]:
        got = _pack(_context(product_raw[1], {"TAE_PFKS_GEMM": variant}), pbs_outputs, variant)
        assert np.array_equal(got, ref), variant


def test_pack_decrypts_to_the_input_bits(packed_auto, client, pbs_outputs):  # noqa: F811
    """Row 0 aside (crafted words), the rows are real ciphertexts: the packed GLWEs carry their phases."""
    got = client.decrypt_packed(tfhe_aes.PackedBits(packed_auto, B_AUTO, "server"))
    want = client.decrypt_bits_raw(pbs_outputs)
    assert np.array_equal(got[1:], want[1:])


def test_pack_chunks_are_whole_glwes(gpu_context):
    """More than the 16384 bits of one chunk of keyswitch scratch: the second chunk reads its bits and writes its
    GLWEs at the right offsets.  Random words stand for the ciphertexts (what they are does not matter here); the
    parts are packed by themselves, the last one on the row-limb path."""
    chunk, tail = 16384, 37
    rows = E.random_words(np.random.default_rng(2026), (chunk + tail, BIG))
    whole = gpu_context.pack(rows).data
    assert whole.shape == (chunk // PN + 1, GLWE)
    assert np.array_equal(whole[:chunk // PN], gpu_context.pack(rows[:chunk]).data)
    assert np.array_equal(whole[chunk // PN:], _pack(gpu_context, rows[chunk:], "rows"))


# ---- the stage call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, want", ((3, "rows"), (B_AUTO, None)))
def test_stage_returns_the_per_bit_glwes(gpu_context, oracle_keys, pbs_outputs, B, want):  # noqa: F811
    want = want or os.environ.get("TAE_PFKS_GEMM", DEFAULT).split(":")[0]
    out = np.full((B, GLWE), 0x5A5A, dtype=U64)
    N.check(N.lib().tae_stage_pack_pfks(gpu_context._h, _vp(pbs_outputs), B, _vp(out), N.TAE_MEM_HOST))
    assert gpu_context.last_pfks_kernel() == want
    for i in (0, B - 1):
        assert np.array_equal(out[i], oracle_keys.pfks(PK, pbs_outputs[i])), (B, i)


# ---- pack, crafted keys ----------------------------------------------------------------------------------------
def crafted_rows(B, limb_model):
    """Random words with decomposer_edge_words in row 0, saturating_coefficient in every word of row 1, body-only
    rows (0, 2^63, 2^64 - 1) in rows 2, B - 2 (B > 4) and B - 1.  The first rows sit in GLWE 0, the last two in the
    last GLWE."""
    rows = E.random_words(np.random.default_rng(77 + B), (B, BIG))
    rows[0] = E.edge_row(16, 2, BIG)
    if B > 2:
        rows[1] = U64(E.saturating_coefficient(16, 2, limb_model))
        bodies = {2: 0, B - 1: E.MASK64}
        if B > 4:
            bodies[B - 2] = 1 << 63
        for r, body in bodies.items():
            rows[r] = 0
            rows[r, -1] = U64(body)
    return rows


@pytest.fixture(scope="module")
def crafted(oracle_mod, product_raw):
    """Per crafted key: the raw arrays (a zero bootstrapping key: nothing here bootstraps), the oracle on them and a
    default context."""
    sets = {}

    def get(key):
        if key not in sets:
            ksk, bsk, pfpksk = product_raw[1]
            make = {"pattern": E.pattern_key, "saturating": E.saturating_key}[key]
            raw = (make(len(ksk)), np.zeros(len(bsk), dtype=U64), make(len(pfpksk)))
            sets[key] = (raw, oracle_mod.Keys(PID, None, raw=raw), _context(raw, {}))
        return sets[key]

    yield get
    sets.clear()


@pytest.mark.parametrize("key", ("pattern", "saturating"))
def test_pack_crafted_keys_equal_oracle(crafted, key):
    raw, ok, ctx = crafted(key)
    small = crafted_rows(3, "rows6")
    got = _pack(ctx, small, "rows")
    assert np.array_equal(got[0], oracle_pack(ok, small)), (key, 3)
    big = crafted_rows(B_AUTO, "kslots")
    got = _pack(ctx, big, os.environ.get("TAE_PFKS_GEMM", DEFAULT).split(":")[0])
    for g in (0, 4):
        assert np.array_equal(got[g], oracle_pack(ok, big[g * PN:(g + 1) * PN])), (key, B_AUTO, g)


# ---- end to end ------------------------------------------------------------------------------------------------
AES_KEY = bytes(range(0x10, 0x20))
IV8 = bytes(range(0xC0, 0xC8))
IV16 = bytes(range(0xA0, 0xB0))
MESSAGE = bytes((7 * i + 3) & 0xFF for i in range(32))  # two blocks


@pytest.fixture(scope="module")
def expanded_key(gpu_context, client):
    """The AES key uploaded packed (one GLWE instead of 128 LWEs), unpacked and expanded on the device."""
    up = aes_128.encrypt_byte_array_packed(client, AES_KEY, start_index=42_000)
    assert up.data.shape == (1, GLWE) and up.count == 128
    return V.key_schedule(gpu_context, gpu_context.unpack(up))


def test_ctr_transcipher_packed_round_trip(gpu_context, client, expanded_key):
    data = aes_var.ctr_xor_plain(AES_KEY, IV8, 1, MESSAGE)
    res = gpu_context.pack(V.ctr_transcipher(gpu_context, expanded_key, IV8, 1, data))
    assert res.origin == "server" and res.count == 256 and res.data.shape == (1, GLWE)
    assert aes_128.decrypt_byte_array_packed(client, res) == MESSAGE
    wire = tfhe_aes.PackedBits.from_narrow(res.narrow(), res.count, "server")
    assert aes_128.decrypt_byte_array_packed(client, wire) == MESSAGE


def test_round_trip_through_the_32_bit_wire_form(gpu_context, client):
    """Upload and result both cross as 32-bit words."""
    up = aes_128.encrypt_byte_array_packed(client, AES_KEY, start_index=42_100)
    up = tfhe_aes.PackedBits.from_narrow(up.narrow(), up.count, "client", up.group)
    ek = V.key_schedule(gpu_context, gpu_context.unpack(up))
    data = aes_var.ctr_xor_plain(AES_KEY, IV8, 1, MESSAGE)
    res = gpu_context.pack(V.ctr_transcipher(gpu_context, ek, IV8, 1, data))
    res = tfhe_aes.PackedBits.from_narrow(res.narrow(), res.count, "server")
    assert aes_128.decrypt_byte_array_packed(client, res) == MESSAGE


def test_cbc_transcipher_packed_round_trip(gpu_context, client, expanded_key):
    data = aes_var.cbc_encrypt_plain(AES_KEY, IV16, MESSAGE)[:32]
    dk = V.decrypt_key(gpu_context, expanded_key)
    res = gpu_context.pack(V.cbc_transcipher(gpu_context, dk, IV16, data))
    assert aes_128.decrypt_byte_array_packed(client, res) == MESSAGE


def test_device_resident_pack_equals_host_arrays(gpu_context, client):
    torch = pytest.importorskip("torch")
    rk = client.encrypt_bits_raw([b for byte in b"".join(aes_var.key_schedule_plain(AES_KEY)) for b in aes_128.u8_to_bits(byte)],
                                 start_index=42_200_000)
    data = aes_var.ctr_xor_plain(AES_KEY, IV8, 1, MESSAGE)
    host = gpu_context.pack(V.ctr_transcipher_raw(gpu_context, rk, IV8, 1, data))
    assert aes_128.decrypt_byte_array_packed(client, host) == MESSAGE
    d_rk = torch.from_numpy(rk.view(np.int64)).cuda()
    d_bits = torch.zeros((256, BIG), dtype=torch.int64, device="cuda")
    d_out = torch.full((1, GLWE), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    V.ctr_transcipher_device(gpu_context, 128, d_rk.data_ptr(), IV8, 1, data, 10, d_bits.data_ptr())
    gpu_context.pack_device(d_bits.data_ptr(), 256, d_out.data_ptr())
    assert np.array_equal(d_out.cpu().numpy().view(U64), host.data)


# ---- parameter sets --------------------------------------------------------------------------------------------
def test_other_parameter_sets_answer_param(gpu_context8):
    bits = np.zeros((2, gpu_context8.lwe_size), dtype=U64)
    out = np.zeros((1, GLWE), dtype=U64)
    for fn in ("tae_pack_bits_raw", "tae_unpack_bits_raw", "tae_stage_pack_pfks"):
        code = getattr(N.lib(), fn)(gpu_context8._h, _vp(bits), 2, _vp(out), N.TAE_MEM_HOST)
        assert code == N.TAE_E_PARAM, fn
    assert N.lib().tae_pack_bits_raw(None, _vp(bits), 2, _vp(out), N.TAE_MEM_HOST) == N.TAE_E_ARG
