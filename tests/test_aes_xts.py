"""XTS-AES without a GPU (include/tfhe_aes_gpu.h "XTS-AES decryption"):

- the plain model against IEEE 1619 vectors, ranges inside a data unit and 32-byte keys;
- the row weights w(j) of the mask matrices against the table of DESIGN.md 5.12 and against this file's own
  restatement (the byte-wise alpha step applied j times to the 128 unit vectors);
- the noise rule: max index 4095 passes and 65535 is TAE_E_NOISE at params_sqrd_lvl_64, the other models are
  TAE_E_PARAM, and the weights place the limit where the design says;
- argument errors before the device, then TAE_E_NODEV without one;
- the mask layer host-compiled (tests/native/aes_xts_test.cpp), plain and as a stand-alone
  -fsanitize=address,undefined binary;
- the host model's per-bit levels and ids, called in the product library (tests/native/aes_xts_noise_test.cpp).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_var

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PID = tfhe_aes.PARAMS_SQRD_LVL_64
W = 32

# IEEE 1619 vectors 1, 2 and 4: (key1, key2, data-unit number, plaintext, ciphertext or its two ends)
ZERO = bytes(16)
VEC1 = (ZERO, ZERO, 0, bytes(32),
        bytes.fromhex("917cf69ebd68b2ec9b9fe9a3eadda692cd43d2f59598ed858c02c2652fbf922e"))
VEC2 = (bytes([0x11] * 16), bytes([0x22] * 16), 0x3333333333, bytes([0x44] * 32),
        bytes.fromhex("c454185e6a16936e39334038acef838bfb186fff7480adc4289382ecd6d394f0"))
KEY1_4 = bytes.fromhex("27182818284590452353602874713526")
KEY2_4 = bytes.fromhex("31415926535897932384626433832795")
PT4 = bytes(range(256)) * 2
CT4_HEAD = bytes.fromhex("27a7479befa1d476489f308cd4cfa6e2a96e4bbe3208ff25287dd3819616e89c")
CT4_TAIL = bytes.fromhex("0a282df920147beabe421ee5319d0568")
WEIGHTS = {0: 1, 1: 2, 2: 3, 8: 4, 121: 4, 122: 5, 127: 7, 128: 7, 255: 9, 4095: 14, 65535: 81}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


# ---- plain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", (VEC1, VEC2), ids=("vector1", "vector2"))
def test_ieee_vectors(vec):
    key1, key2, unit, pt, ct = vec
    assert aes_var.xts_encrypt_plain(key1, key2, unit, pt) == ct
    assert aes_var.xts_decrypt_plain(key1, key2, unit, ct) == pt
    assert aes_var.xts_decrypt_plain(key1, key2, unit.to_bytes(16, "little"), ct) == pt
    assert aes_var.xts_decrypt_plain(key1, key2, unit, ct[16:], first_block=1) == pt[16:]
    assert aes_var.xts_encrypt_plain(key1, key2, unit, pt[16:], first_block=1) == ct[16:]


def test_ieee_vector_512_bytes():
    ct = aes_var.xts_encrypt_plain(KEY1_4, KEY2_4, 0, PT4)
    assert len(ct) == 512 and ct[:32] == CT4_HEAD and ct[-16:] == CT4_TAIL
    assert aes_var.xts_decrypt_plain(KEY1_4, KEY2_4, 0, ct) == PT4
    assert aes_var.xts_decrypt_plain(KEY1_4, KEY2_4, 0, ct[256:], first_block=16) == PT4[256:]


def test_32_byte_keys():
    key1, key2 = bytes(range(32)), bytes(range(0x40, 0x60))
    tweak = bytes(range(0xF0, 0x100))
    msg = bytes((17 * i + 9) & 255 for i in range(48))
    ct = aes_var.xts_encrypt_plain(key1, key2, tweak, msg)
    assert ct != msg and aes_var.xts_decrypt_plain(key1, key2, tweak, ct) == msg
    # block 1 composed by hand from the block cipher: M_1 = alpha Enc_K2(tweak)
    ek1, ek2 = aes_var.key_schedule_plain(key1), aes_var.key_schedule_plain(key2)
    assert len(ek1) == 60
    t = int.from_bytes(aes_var.encrypt_block_plain(ek2, tweak), "little") << 1
    m1 = ((t & ((1 << 128) - 1)) ^ (0x87 if t >> 128 else 0)).to_bytes(16, "little")
    x = aes_var.encrypt_block_plain(ek1, bytes(a ^ b for a, b in zip(msg[16:32], m1)))
    assert bytes(a ^ b for a, b in zip(x, m1)) == ct[16:32]


def test_plain_argument_errors():
    for call in (lambda: aes_var.xts_encrypt_plain(ZERO, bytes(32), 0, bytes(16)),
                 lambda: aes_var.xts_encrypt_plain(ZERO, ZERO, 0, bytes(17)),
                 lambda: aes_var.xts_decrypt_plain(ZERO, ZERO, 0, b""),
                 lambda: aes_var.xts_decrypt_plain(ZERO, ZERO, bytes(15), bytes(16))):
        with pytest.raises(ValueError):
            call()


# ---- row weights ------------------------------------------------------------------------------------------------
def _alpha(t):
    """IEEE 1619 5.2 on rows of 16 bytes [n][16]: every byte shifted left by one with the carry of the byte before
    it, 0x87 into byte 0 on carry out of byte 15."""
    out = (t << 1) & 0xFF
    out[:, 1:] |= t[:, :-1] >> 7
    out[:, 0] ^= 0x87 * (t[:, 15] >> 7)
    return out


def _weights_by_stepping(last):
    """w(j) for j = 0..last: the images of the 128 unit vectors stepped together, rows counted per output bit."""
    t = np.zeros((128, 16), dtype=np.uint16)
    for src in range(128):
        t[src, src >> 3] = 0x80 >> (src & 7)
    out = []
    for _ in range(last + 1):
        out.append(int(np.unpackbits(t.astype(np.uint8), axis=1).sum(axis=0).max()))
        t = _alpha(t)
    return out


def test_row_weights():
    stepped = _weights_by_stepping(65535)
    for j, w in WEIGHTS.items():
        assert aes_var.xts_row_weight(j) == w == stepped[j], j
    for j in (7, 126, 243, 244, 256, 300, 511, 1023, 40000):
        assert aes_var.xts_row_weight(j) == stepped[j], j
    # where the unrefreshed tweak would stop (9 + 9 w <= 64: w <= 6) and what 4 KiB sectors need
    assert next(j for j, w in enumerate(stepped) if w > 6) == 127
    assert next(j for j, w in enumerate(stepped) if w > 7) == 244
    assert max(stepped[:32]) == 4 and max(stepped[:256]) == 9  # 512-byte and 4 KiB sectors
    # w(j) is not monotonic: the noise rule (w <= 55 at params_sqrd_lvl_64) first fails at block 1721
    assert stepped[511] == 11 and max(stepped[:512]) == 16
    assert next(j for j, w in enumerate(stepped) if w > 55) == 1721


# ---- noise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bits, rounds", ((128, 10), (192, 12), (256, 14), (128, 1)))
def test_noise_schedule(key_bits, rounds):
    aes_var.xts_noise_schedule_check(PID, key_bits, rounds, 4095)
    assert _code(lambda: aes_var.xts_noise_schedule_check(PID, key_bits, rounds, 65535)) == N.TAE_E_NOISE


def test_noise_schedule_limit_follows_the_weights():
    """9 + w(j) <= 64 at params_sqrd_lvl_64: passes exactly where w(j) <= 55."""
    stepped = _weights_by_stepping(20000)
    first_bad = next(j for j, w in enumerate(stepped) if w > 55)
    aes_var.xts_noise_schedule_check(PID, 128, 10, first_bad - 1)
    assert _code(lambda: aes_var.xts_noise_schedule_check(PID, 128, 10, first_bad)) == N.TAE_E_NOISE


def test_noise_schedule_parameter_errors():
    for pid in (tfhe_aes.PARAMS_WOPPBS_8BIT, tfhe_aes.PARAMS_SHORTINT_1BIT):
        assert _code(lambda: aes_var.xts_noise_schedule_check(pid, 128, 10, 0)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.xts_noise_schedule_check(PID, 160, 10, 0)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.xts_noise_schedule_check(PID, 128, 11, 0)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.xts_noise_schedule_check(PID, 256, 0, 0)) == N.TAE_E_PARAM


# ---- entry points -----------------------------------------------------------------------------------------------
def test_compute_calls_check_arguments_then_the_device():
    """len == 0 and len == 17 are TAE_E_PARAM and null arrays TAE_E_ARG before anything else; a machine without a GPU
    then answers TAE_E_NODEV (it has no context to pass), one with a GPU rejects the null context."""
    L = N.lib()
    key = np.zeros((44 * W, 4), dtype=np.uint64)
    out = np.zeros((32 * 8, 4), dtype=np.uint64)
    handles = (C.c_void_p * (44 * W))()
    outs = (C.c_void_p * 256)()
    no_context = N.TAE_E_NODEV if tfhe_aes.device_count() == 0 else N.TAE_E_ARG

    def raw(units, key_bits=128):
        arr, keep, _ = aes_var._xts_units(units)
        return L.tae_aesx_xts_transcipher_raw(None, key_bits, _vp(key), _vp(key), arr, len(units), 10, _vp(out),
                                              N.TAE_MEM_HOST)

    def bits(units):
        arr, keep, _ = aes_var._xts_units(units)
        return L.tae_aesx_xts_transcipher(None, 128, handles, handles, arr, len(units), 10, outs)

    for call in (raw, bits):
        assert call([(0, bytes(17))]) == N.TAE_E_PARAM
        assert call([(0, b"")]) == N.TAE_E_PARAM
        assert call([(0, bytes(16)), (1, bytes(40), 3)]) == N.TAE_E_PARAM
        assert call([(0, bytes(32))]) == no_context
    assert raw([(0, bytes(16))], key_bits=160) == N.TAE_E_PARAM
    arr, keep, _ = aes_var._xts_units([(0, bytes(16))])
    assert L.tae_aesx_xts_transcipher_raw(None, 128, None, _vp(key), arr, 1, 10, _vp(out), N.TAE_MEM_HOST) == N.TAE_E_ARG
    tweaks = np.zeros((2, 16), dtype=np.uint8)
    t_out = np.zeros((2, 128, 4), dtype=np.uint64)
    assert L.tae_aesx_xts_tweaks_raw(None, 128, _vp(key), _vp(tweaks), 2, 10, _vp(t_out), N.TAE_MEM_HOST) == no_context
    assert L.tae_aesx_xts_tweaks_raw(None, 128, None, _vp(tweaks), 2, 10, _vp(t_out), N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesx_xts_tweaks_raw(None, 100, _vp(key), _vp(tweaks), 2, 10, _vp(t_out), N.TAE_MEM_HOST) == N.TAE_E_PARAM
    unit = np.zeros(2, dtype=np.int32)
    index = np.arange(2, dtype=np.uint64)
    assert L.tae_stage_xts_masks(None, _vp(t_out), 2, _vp(unit), _vp(index), 2, _vp(t_out), N.TAE_MEM_HOST) == no_context
    assert L.tae_stage_xts_masks(None, _vp(t_out), 2, None, _vp(index), 2, _vp(t_out), N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesx_xts_row_weight(0, None) == N.TAE_E_ARG


# ---- the mask layer, host-compiled ------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_mask_layer_native(tmp_path, flags):
    exe = str(tmp_path / "aes_xts_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "aes_xts_test.cpp"),
                    os.path.join(ROOT, "tfhe-aes-2_amd", "csrc", "aes_plain.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_noise_levels_and_ids_native(tmp_path):
    """The host model's per-bit bookkeeping, called in the product library without a GPU: level 9 + w(j) and the ids
    of the row's tweak bits for j in {0, 31, 127}, TAE_E_INDEP for outputs that share a tweak bit
    (tests/native/aes_xts_noise_test.cpp)."""
    exe = str(tmp_path / "aes_xts_noise_test")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tfhe-aes-2_amd")], check=True)
    lib = os.path.join(ROOT, "tfhe-aes-2_amd", "tfhe_aes")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "aes_xts_noise_test.cpp"),
                    os.path.join(lib, "libtfhe_aes_amd.so"), "-o", exe, "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
