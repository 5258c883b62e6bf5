"""Packed ciphertext I/O without a GPU (include/tfhe_aes_gpu.h "packed ciphertext I/O"):

- the index maps of csrc/glwe_pack.hpp, host-compiled (tests/native/glwe_pack_test.cpp), plain and as a stand-alone
  -fsanitize=address,undefined binary;
- the client side: packed encryption and decryption, the stream layout of the new purpose, the 32-bit wire form,
  the host extraction decrypting under the oracle, the noise of an upload;
- the design, on the oracle alone: sum_j X^j Keys.pfks(k, ct_j) of 512 fresh bits decrypts to the bits and adds less
  than 2^44 to any coefficient's phase, narrowed to 32 bits or not;
- argument errors, the other parameter sets (TAE_E_PARAM) and the server calls without a device (TAE_E_NODEV).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_128
from tests.conftest import ENC_SEED, SEED
from tests.packed_ref import BIG, GLWE, PK, PN, U64, extract_np, glwe_phase_np, oracle_pfks_rows, rotate_np, signed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PID = tfhe_aes.PARAMS_SQRD_LVL_64
COUNTS = (1, 511, 512, 513, 1030)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the index maps, host-compiled -----------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_index_maps_native(tmp_path, flags):
    exe = str(tmp_path / "glwe_pack_test")
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, os.path.join(ROOT, "tests", "native", "glwe_pack_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


# ---- client ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def client(product_raw):
    return product_raw[0]


@pytest.mark.parametrize("count", COUNTS)
def test_packed_round_trip(client, count):
    bits = np.random.default_rng(count).integers(0, 2, size=count).astype(np.uint8)
    up = client.encrypt_packed(bits, start_index=10)
    assert up.origin == "client" and up.count == count
    assert up.data.shape == ((count + PN - 1) // PN, GLWE) == tuple(
        [tfhe_aes.packed_len(PID, count)[0], tfhe_aes.packed_len(PID, count)[1] // tfhe_aes.packed_len(PID, count)[0]])
    assert np.array_equal(client.decrypt_packed(up), bits)
    wire = up.narrow()
    assert wire.dtype == np.uint32 and wire.shape == up.data.shape
    assert np.array_equal(wire, ((up.data + U64(1 << 31)) >> U64(32)).astype(np.uint32))
    back = tfhe_aes.PackedBits.from_narrow(wire, count, "client")
    assert np.array_equal(back.data, wire.astype(U64) << U64(32))
    assert np.array_equal(client.decrypt_packed(back), bits)


def test_unused_coefficients_carry_zero(client):
    up = client.encrypt_packed([1] * 5, start_index=11)
    phase = signed(glwe_phase_np(up.data[0], client.secrets()[1]))
    assert np.all(np.abs(phase[5:]) < 1 << 20)  # zero plus glwe noise (std 2^12)
    assert np.all(np.abs(signed(U64(phase[:5].view(U64) - U64(1 << 63)))) < 1 << 20)


def test_byte_arrays_are_msb_first(client):
    msg = bytes([0x80, 0x01, 0xA5])
    up = aes_128.encrypt_byte_array_packed(client, msg, start_index=12)
    assert up.count == 24 and up.group == 8
    assert list(client.decrypt_packed(up)[:16]) == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert aes_128.decrypt_byte_array_packed(client, up) == msg


def test_streams_of_the_packed_purpose(client):
    """The same seed and index give the same words; another index, and the per-bit ENCRYPT stream of the same index,
    give other masks; explicit and automatic indices do not alias."""
    bits = np.arange(600) & 1
    a = client.encrypt_packed(bits, start_index=20)
    again = tfhe_aes.client_key_from_seed(PID, SEED).encrypt_packed(bits, start_index=20)
    assert np.array_equal(a.data, again.data)
    b = client.encrypt_packed(bits, start_index=21)
    # GLWE 1 of the first call and GLWE 0 of the second are both packed encryption #21: the same mask
    assert np.array_equal(a.data[1, :PK * PN], b.data[0, :PK * PN])
    assert not np.any(a.data[0, :PK * PN] == b.data[0, :PK * PN])
    per_bit = client.encrypt_bits_raw([0, 1], start_index=20)  # the K mask words of LWE #20 and #21
    assert not np.any(per_bit[0, :-1] == a.data[0, :PK * PN])
    assert not np.any(per_bit[1, :-1] == a.data[1, :PK * PN])
    auto1, auto2 = client.encrypt_packed(bits), client.encrypt_packed(bits)
    for other in (auto2.data, a.data, b.data):
        assert not np.any(auto1.data[:, :PK * PN] == other[:, :PK * PN])
    assert np.array_equal(client.decrypt_packed(auto1), bits)
    with pytest.raises(tfhe_aes.TaeError) as e:
        client.encrypt_packed(bits, start_index=(1 << 63) - 1)  # two GLWEs: the second index is out of range
    assert e.value.code == N.TAE_E_ARG


def test_host_extraction_decrypts_under_the_oracle(client, oracle_keys):
    bits = np.random.default_rng(5).integers(0, 2, size=700).astype(np.uint8)
    up = client.encrypt_packed(bits, start_index=30)
    lwes = extract_np(up.data, 700)
    assert np.array_equal(oracle_keys.decrypt_bits(lwes), bits)
    assert np.array_equal(client.decrypt_bits_raw(lwes), bits)
    # the extraction is exact: the LWE's phase is the GLWE's coefficient
    glwe_sk = client.secrets()[1]
    for g in range(2):
        phase = glwe_phase_np(up.data[g], glwe_sk)
        for j in (0, 1, 187, 511 if g == 0 else 187):
            assert oracle_keys.phase(lwes[g * PN + j]) == int(phase[j]), (g, j)


def test_upload_noise_is_glwe_noise(client):
    """The phase error of 8 packed GLWEs (4096 coefficients) has the std of glwe_std.  The sample std of n Gaussian
    draws has relative std 1 / sqrt(2 n) = 1.1%; the bound is five of those.  (Rounding to integers adds 1/12 to a
    variance of 4086^2.)"""
    n = 8 * PN
    bits = np.random.default_rng(9).integers(0, 2, size=n).astype(np.uint8)
    up = client.encrypt_packed(bits, start_index=50)
    glwe_sk = client.secrets()[1]
    phase = np.concatenate([glwe_phase_np(g, glwe_sk) for g in up.data])
    err = signed(phase - (bits.astype(U64) << U64(63))).astype(np.float64)
    want = client.params["glwe_std"] * 2.0 ** 64
    print(f"upload noise: std {err.std():.1f}, glwe_std 2^64 = {want:.1f}, mean {err.mean():.1f}")
    assert abs(err.std() / want - 1) < 5 / np.sqrt(2 * n)
    assert abs(err.mean()) < 5 * want / np.sqrt(n)
    assert want < client.params["lwe_std"] * 2.0 ** 64  # below a fresh bit's noise: noise level 1 is an upper bound


# ---- the design, on the oracle alone ---------------------------------------------------------------------------
def test_design_pin_pack_of_fresh_bits(oracle_keys):
    """sum_j X^j pfks(k, ct_j) of 512 fresh bits: the sign convention (it decrypts to the bits) and the added error
    per coefficient, packed phase minus the input LWE's phase.  The bound 2^44 is derived: 2^18 under the decode
    margin 2^62, 2^5.6 under the fresh noise std 2^49.65.  It holds after rounding to the 32-bit wire form too."""
    bits = np.random.default_rng(64).integers(0, 2, size=PN).astype(np.uint8)
    cts = oracle_keys.encrypt_bits(bits, ENC_SEED, start_index=70_000)
    packed = np.zeros(GLWE, dtype=U64)
    for j, g in enumerate(oracle_pfks_rows(oracle_keys, cts)):
        packed += rotate_np(g, j)
    glwe_sk = oracle_keys.glwe_sk()
    in_phase = np.array([oracle_keys.phase(ct) for ct in cts], dtype=U64)
    for name, words in (("u64", packed), ("32-bit wire", ((packed + U64(1 << 31)) >> U64(32)) << U64(32))):
        phase = glwe_phase_np(words, glwe_sk)
        decoded = ((phase + U64(1 << 62)) >> U64(63)).astype(np.uint8)
        assert np.array_equal(decoded, bits), name
        added = signed(phase - in_phase).astype(np.float64)
        print(f"{name}: added error std 2^{np.log2(added.std()):.2f}, max 2^{np.log2(np.abs(added).max()):.2f}")
        assert np.abs(added).max() < 2.0 ** 44, name


# ---- argument errors -------------------------------------------------------------------------------------------
def test_packed_len_and_parameter_sets():
    assert tfhe_aes.packed_len(PID, 1) == (1, GLWE) and tfhe_aes.packed_len(PID, 513) == (2, 2 * GLWE)
    g = C.c_size_t()
    for pid in (tfhe_aes.PARAMS_SQRD_LVL_1, tfhe_aes.PARAMS_SQRD_LVL_4, tfhe_aes.PARAMS_SQRD_LVL_256,
                tfhe_aes.PARAMS_WOPPBS_8BIT, tfhe_aes.PARAMS_SHORTINT_1BIT, 99):
        assert N.lib().tae_packed_len(pid, 8, C.byref(g), None) == N.TAE_E_PARAM, pid
    assert N.lib().tae_packed_len(PID, 0, C.byref(g), None) == N.TAE_E_ARG


def test_client_calls_reject_other_sets_and_bad_arguments(client):
    L = N.lib()
    bits = np.array([0, 1, 1], dtype=np.uint8)
    out = np.zeros((1, GLWE), dtype=U64)
    for pid in (tfhe_aes.PARAMS_SQRD_LVL_4, tfhe_aes.PARAMS_WOPPBS_8BIT, tfhe_aes.PARAMS_SHORTINT_1BIT):
        other = tfhe_aes.client_key_from_seed(pid, SEED)
        assert L.tae_encrypt_packed_raw(other._h, _vp(bits), 3, 0, _vp(out)) == N.TAE_E_PARAM, pid
        assert L.tae_decrypt_packed_raw(other._h, _vp(out), 3, _vp(bits)) == N.TAE_E_PARAM, pid
    assert L.tae_encrypt_packed_raw(client._h, _vp(bits), 0, 0, _vp(out)) == N.TAE_E_ARG
    assert L.tae_encrypt_packed_raw(client._h, None, 3, 0, _vp(out)) == N.TAE_E_ARG
    assert L.tae_encrypt_packed_raw(client._h, _vp(bits), 3, 0, None) == N.TAE_E_ARG
    assert L.tae_encrypt_packed_raw(None, _vp(bits), 3, 0, _vp(out)) == N.TAE_E_ARG
    assert L.tae_encrypt_packed_raw(client._h, _vp(np.array([0, 2], dtype=np.uint8)), 2, 0, _vp(out)) == N.TAE_E_ARG
    assert L.tae_encrypt_packed_raw(client._h, _vp(bits), 3, 1 << 63, _vp(out)) == N.TAE_E_ARG
    assert L.tae_decrypt_packed_raw(client._h, _vp(out), 0, _vp(bits)) == N.TAE_E_ARG
    assert L.tae_decrypt_packed_raw(client._h, None, 3, _vp(bits)) == N.TAE_E_ARG
    assert L.tae_decrypt_packed_raw(client._h, _vp(out), 3, None) == N.TAE_E_ARG
    narrow = np.zeros(4, dtype=np.uint32)
    assert L.tae_packed_narrow(None, 4, _vp(narrow)) == N.TAE_E_ARG
    assert L.tae_packed_widen(_vp(narrow), 4, None) == N.TAE_E_ARG
    with pytest.raises(ValueError):
        tfhe_aes.PackedBits(out, 513, "client")  # one GLWE cannot hold 513 bits
    with pytest.raises(ValueError):
        tfhe_aes.PackedBits(out, 3, "elsewhere")


def test_server_calls_check_arguments_then_the_device():
    """count == 0 and null arrays are argument errors before anything else; a machine without a GPU then answers
    TAE_E_NODEV (it has no context to pass), one with a GPU rejects the null context."""
    L = N.lib()
    bits = np.zeros((2, BIG), dtype=U64)
    glwes = np.zeros((1, GLWE), dtype=U64)
    handles = (C.c_void_p * 2)()
    calls = {"tae_unpack_bits_raw": lambda a, n, b: L.tae_unpack_bits_raw(None, a, n, b, N.TAE_MEM_HOST),
             "tae_pack_bits_raw": lambda a, n, b: L.tae_pack_bits_raw(None, a, n, b, N.TAE_MEM_HOST),
             "tae_stage_pack_pfks": lambda a, n, b: L.tae_stage_pack_pfks(None, a, n, b, N.TAE_MEM_HOST),
             "tae_unpack_bits": lambda a, n, b: L.tae_unpack_bits(None, a, n, b),
             "tae_pack_bits": lambda a, n, b: L.tae_pack_bits(None, a, n, b)}
    args = {"tae_unpack_bits_raw": (_vp(glwes), _vp(bits)), "tae_pack_bits_raw": (_vp(bits), _vp(glwes)),
            "tae_stage_pack_pfks": (_vp(bits), _vp(np.zeros((2, GLWE), dtype=U64))),
            "tae_unpack_bits": (_vp(glwes), handles), "tae_pack_bits": (handles, _vp(glwes))}
    no_context = N.TAE_E_NODEV if tfhe_aes.device_count() == 0 else N.TAE_E_ARG
    for name, call in calls.items():
        a, b = args[name]
        assert call(a, 0, b) == N.TAE_E_ARG, name
        assert call(None, 2, b) == N.TAE_E_ARG, name
        assert call(a, 2, None) == N.TAE_E_ARG, name
        assert call(a, 2, b) == no_context, name
