"""AES-CCM without a GPU (include/tfhe_aes_gpu.h "AES-CCM decryption"):

- the plain model against RFC 3610 packet vector 1, the CBC-MAC before masking and the four MAC blocks;
- the library's frame layout (tae_aesx_ccm_format) against this module's plain restatement, at the edges of L, M,
  the AAD and the payload, and every refusal;
- the noise rule without a device;
- argument errors of the compute calls;
- the host layer compiled stand-alone (tests/native/aes_ccm_test.cpp: ccm_format, pub_plan, ccm_absorb_word and
  ccm_tag_word), plain and as a -fsanitize=address,undefined binary;
- the host model's per-bit levels and ids, called in the product library (tests/native/aes_ccm_noise_test.cpp).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_multi, aes_var

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PID = tfhe_aes.PARAMS_SQRD_LVL_64
W = 32

# RFC 3610 packet vector 1
KEY = bytes(range(0xC0, 0xD0))
NONCE = bytes.fromhex("00000003020100A0A1A2A3A4A5")
AAD = bytes(range(8))
PAYLOAD = bytes(range(8, 0x1F))
BODY = bytes.fromhex("588C979A61C663D2F066D0C2C0F989806D5F6B61DAC384")
TAG = bytes.fromhex("17E8D12CFDF926E0")
MAC = bytes.fromhex("2DC697E411CA83A8")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


# ---- plain ------------------------------------------------------------------------------------------------------
def test_rfc3610_vector_1():
    assert aes_var.ccm_encrypt_plain(KEY, NONCE, AAD, PAYLOAD, 8) == BODY + TAG
    assert aes_var.ccm_mac_plain(KEY, NONCE, AAD, PAYLOAD, 8) == MAC
    assert len(aes_var._ccm_blocks_plain(NONCE, AAD, PAYLOAD, 8)[1]) == 4
    assert aes_var.ccm_decrypt_plain(KEY, NONCE, AAD, BODY + TAG, 8) == (PAYLOAD, bytes(8))
    # S_0 composed by hand from the block cipher: the tag is the MAC under it
    ek = aes_var.key_schedule_plain(KEY)
    s0 = aes_var.encrypt_block_plain(ek, bytes([1]) + NONCE + bytes(2))
    assert bytes(a ^ b for a, b in zip(MAC, s0)) == TAG


def test_decrypt_plain_reports_the_difference():
    """A flipped tag bit shows at its place; a flipped ciphertext bit changes the payload and the whole MAC."""
    bad_tag = bytearray(BODY + TAG)
    bad_tag[-3] ^= 0x10
    assert aes_var.ccm_decrypt_plain(KEY, NONCE, AAD, bytes(bad_tag), 8) == (PAYLOAD, bytes([0, 0, 0, 0, 0, 0x10, 0, 0]))
    bad_ct = bytearray(BODY + TAG)
    bad_ct[5] ^= 0x10
    payload, diff = aes_var.ccm_decrypt_plain(KEY, NONCE, AAD, bytes(bad_ct), 8)
    assert payload == PAYLOAD[:5] + bytes([PAYLOAD[5] ^ 0x10]) + PAYLOAD[6:] and any(diff)
    for key in (bytes(range(24)), bytes(range(32))):
        data = aes_var.ccm_encrypt_plain(key, NONCE[:7], b"", PAYLOAD, 16)
        assert len(data) == 23 + 16 and aes_var.ccm_decrypt_plain(key, NONCE[:7], b"", data, 16) == (PAYLOAD, bytes(16))
    with pytest.raises(ValueError):
        aes_var.ccm_decrypt_plain(KEY, NONCE, AAD, bytes(7), 8)


# ---- the frame layout -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonce_len, tag_len, aad_len, payload_len",
                         ((13, 8, 8, 23), (7, 16, 0, 16), (13, 4, 0, 17), (13, 8, 14, 0), (13, 8, 15, 0), (7, 4, 15, 17),
                          (13, 16, 0, 0), (10, 6, 300, 33)))
def test_format_equals_plain_restatement(nonce_len, tag_len, aad_len, payload_len):
    nonce = bytes(range(0x20, 0x20 + nonce_len))
    aad = bytes((5 * i + 1) & 255 for i in range(aad_len))
    payload = bytes((3 * i + 7) & 255 for i in range(payload_len))
    ctr, mac, src = aes_var.ccm_format(nonce, aad, payload_len, tag_len)
    ell, want_mac, want_ctr = aes_var._ccm_blocks_plain(nonce, aad, payload, tag_len)
    assert ell == 15 - nonce_len
    assert [bytes(a) for a in ctr] == want_ctr and len(ctr) == 1 + (payload_len + 15) // 16
    aad_blocks = (2 + aad_len + 15) // 16 if aad_len else 0
    assert len(mac) == len(want_mac) == 1 + aad_blocks + (payload_len + 15) // 16
    # the payload bytes in their slots, everything else public with the restatement's value
    filled = mac.copy()
    filled[src >= 0] = np.frombuffer(payload, dtype=np.uint8)[src[src >= 0]]
    assert [bytes(b) for b in filled] == want_mac
    assert np.array_equal(np.sort(src[src >= 0]), np.arange(payload_len))
    assert not mac[src >= 0].any() and (src >= -1).all()
    assert bool(mac[0, 0] & 64) == bool(aad_len)


def test_format_refusals():
    nonce = bytes(13)
    for call in (lambda: aes_var.ccm_format(bytes(6), b"", 0, 8), lambda: aes_var.ccm_format(bytes(14), b"", 0, 8),
                 lambda: aes_var.ccm_format(nonce, b"", 0, 7), lambda: aes_var.ccm_format(nonce, b"", 0, 2),
                 lambda: aes_var.ccm_format(nonce, b"", 0, 18), lambda: aes_var.ccm_format(nonce, bytes(0xFF00), 0, 8),
                 lambda: aes_var.ccm_format(nonce, b"", 1 << 16, 8)):
        assert _code(call) == N.TAE_E_PARAM
    assert len(aes_var.ccm_format(nonce, bytes(0xFEFF), 0, 8)[1]) == 1 + (2 + 0xFEFF + 15) // 16
    assert len(aes_var.ccm_format(bytes(12), b"", 1 << 16, 8)[0]) == 1 + 4096
    for call in (lambda: aes_var._ccm_blocks_plain(bytes(6), b"", b"", 8),
                 lambda: aes_var._ccm_blocks_plain(nonce, b"", b"", 5),
                 lambda: aes_var._ccm_blocks_plain(nonce, bytes(0xFF00), b"", 8),
                 lambda: aes_var._ccm_blocks_plain(nonce, b"", bytes(1 << 16), 8)):
        with pytest.raises(ValueError):
            call()


# ---- noise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bits, rounds", ((128, 10), (192, 12), (256, 14), (128, 2)))
def test_noise_schedule(key_bits, rounds):
    aes_var.ccm_noise_schedule_check(PID, key_bits, rounds)


def test_noise_schedule_parameter_errors():
    for pid in (tfhe_aes.PARAMS_WOPPBS_8BIT, tfhe_aes.PARAMS_SHORTINT_1BIT):
        assert _code(lambda: aes_var.ccm_noise_schedule_check(pid, 128, 10)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.ccm_noise_schedule_check(PID, 160, 10)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.ccm_noise_schedule_check(PID, 128, 11)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.ccm_noise_schedule_check(PID, 128, 1)) == N.TAE_E_PARAM  # B_0 and A_0 share groups
    assert _code(lambda: aes_var.ccm_noise_schedule_check(PID, 256, 0)) == N.TAE_E_PARAM
    # the cap is enforced: 4 is below every level of the schedule
    assert _code(lambda: aes_var.ccm_noise_schedule_check(tfhe_aes.PARAMS_SQRD_LVL_4, 128, 10)) == N.TAE_E_NOISE


# ---- entry points -----------------------------------------------------------------------------------------------
def test_compute_calls_reject_null_arguments():
    L = N.lib()
    key = np.zeros((44 * W, 4), dtype=np.uint64)
    out = np.zeros((64, 4), dtype=np.uint64)
    nonce = np.zeros(13, dtype=np.uint8)
    data = np.zeros(16, dtype=np.uint8)
    assert L.tae_aesx_ccm_transcipher_raw(None, 128, _vp(key), _vp(nonce), 13, None, 0, _vp(data), 16, 8, 10, _vp(out),
                                          _vp(out), N.TAE_MEM_HOST) == N.TAE_E_ARG
    arr, _keep, _ = aes_multi._ccm_streams([(0, bytes(13), b"", bytes(16))], 8)
    assert L.tae_aesm_ccm_transcipher_raw(None, 128, _vp(key), 1, arr, 1, 8, 10, _vp(out), _vp(out),
                                          N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesm_pub_keystream_raw(None, 128, _vp(key), 1, None, _vp(data), 1, 10, _vp(out),
                                        N.TAE_MEM_HOST) == N.TAE_E_ARG
    n = C.c_size_t(0)
    assert L.tae_aesx_ccm_format(None, 13, 8, None, 0, 0, C.byref(n), C.byref(n), None, None, None) == N.TAE_E_ARG
    assert L.tae_aesx_ccm_format(_vp(nonce), 13, 8, None, 3, 0, C.byref(n), C.byref(n), None, None, None) == N.TAE_E_ARG


# ---- the host layer, compiled stand-alone -----------------------------------------------------------------------
@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_ccm_layer_native(tmp_path, flags):
    exe = str(tmp_path / "aes_ccm_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "aes_ccm_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_noise_levels_and_ids_native(tmp_path):
    """The host model's per-bit bookkeeping, called in the product library without a GPU: the levels of DESIGN.md
    5.13, the ids of the output bits, the legal XORs and rounds = 1 refused (tests/native/aes_ccm_noise_test.cpp)."""
    exe = str(tmp_path / "aes_ccm_noise_test")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tfhe-aes-2_amd")], check=True)
    lib = os.path.join(ROOT, "tfhe-aes-2_amd", "tfhe_aes")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "aes_ccm_noise_test.cpp"),
                    os.path.join(lib, "libtfhe_aes_amd.so"), "-o", exe, "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
