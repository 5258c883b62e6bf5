"""AES-GCM without a GPU (include/tfhe_aes_gpu.h "AES-GCM decryption"):

- the plain model against test cases 1 - 4 of the GCM specification, and GHASH as a sum of powers;
- the library's frame layout (tae_aesx_gcm_format) and tag rows against tests/gcm_ref.py, at the edges;
- the refusals and the argument errors of the compute calls;
- the noise table of DESIGN.md 5.14, restated from the test's own byte-wise "times x";
- the host layer compiled stand-alone on plain bits (tests/native/aes_gcm_test.cpp), plain and as a
  -fsanitize=address,undefined binary;
- the host model's per-bit levels and ids, called in the product library (tests/native/aes_gcm_noise_test.cpp).
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import tfhe_aes
from tfhe_aes import _native as N
from tfhe_aes import aes_var
from tests import gcm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PID = tfhe_aes.PARAMS_SQRD_LVL_64
W = 32


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _code(call):
    with pytest.raises(tfhe_aes.TaeError) as e:
        call()
    return e.value.code


# ---- plain ------------------------------------------------------------------------------------------------------
def test_specification_cases_1_to_4():
    z = bytes(16)
    assert aes_var.gcm_encrypt_plain(z, bytes(12), b"", b"") == bytes.fromhex("58e2fccefa7e3061367f1d57a4e7455a")
    assert aes_var.encrypt_block_plain(aes_var.key_schedule_plain(z), z) == R.H1
    assert aes_var.gcm_encrypt_plain(z, bytes(12), b"", z) == bytes.fromhex(
        "0388dace60b6a392f328c2b971b2fe78" "ab6e47d42cec13bdf53a67b21257bddf")
    assert aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, b"", R.PT3)[-16:] == R.TAG3
    data = aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, R.AAD4, R.PT3[:60])
    assert data[-16:] == R.TAG4
    assert aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, R.AAD4, data) == (R.PT3[:60], bytes(16))
    assert aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, R.AAD4, R.PT3[:60], 12) == data[:60] + R.TAG4[:12]


def test_decrypt_plain_reports_the_difference():
    data = bytearray(aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, R.AAD4, R.PT3[:60]))
    data[-3] ^= 0x10
    plain, diff = aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, R.AAD4, bytes(data))
    assert plain == R.PT3[:60] and diff == bytes(13) + b"\x10" + bytes(2)
    data[-3] ^= 0x10
    data[5] ^= 0x10
    plain, diff = aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, R.AAD4, bytes(data))
    assert plain[5] == R.PT3[5] ^ 0x10 and any(diff)
    for bad in (lambda: aes_var.gcm_encrypt_plain(R.KEY3, bytes(16), b"", b""),
                lambda: aes_var.gcm_encrypt_plain(R.KEY3, R.IV3, b"", b"", 5),
                lambda: aes_var.gcm_decrypt_plain(R.KEY3, R.IV3, b"", bytes(7), 8)):
        with pytest.raises(ValueError):
            bad()


def test_field_and_ghash_as_a_sum_of_powers():
    rnd = random.Random(5)
    a, b = bytes(rnd.randrange(256) for _ in range(16)), bytes(rnd.randrange(256) for _ in range(16))
    assert aes_var.gf128_mul_plain(a, b) == R.mul(a, b) == R.mul(b, a)
    assert R.mul(a, R.ONE) == a and R.times_x(bytes(15) + b"\x01") == b"\xe1" + bytes(15)
    aad, c = bytes(rnd.randrange(256) for _ in range(20)), bytes(rnd.randrange(256) for _ in range(37))
    xs = R.hashed_blocks(aad, c)
    m, acc, p = len(xs), bytes(16), R.H1
    powers = []
    for _ in range(m):
        powers.append(p)
        p = R.mul(p, R.H1)
    for i, x in enumerate(xs, start=1):
        acc = bytes(u ^ v for u, v in zip(acc, R.mul(x, powers[m - i])))
    assert m == 6 and aes_var.ghash_plain(R.H1, aad, c) == acc
    # the same sum by the tag rows on plain bits
    bits = [bit for q in powers for bit in R.coefs(q)]
    rows = R.tag_rows(aad, c, 16)
    assert R.from_coefs([sum(bits[s] for s in row) & 1 for row in rows]) == acc


# ---- the frame layout -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aad_len,data_len", ((0, 0), (0, 15), (15, 16), (16, 17), (17, 0), (20, 60)))
def test_format_matches_the_restatement(aad_len, data_len):
    aad, c = bytes(range(1, 1 + aad_len)), bytes((7 * i + 3) & 255 for i in range(data_len))
    pub, hashed = aes_var.gcm_format(R.IV3, aad, c, 16)
    n_blk = (data_len + 15) // 16
    assert pub.shape == (2 + n_blk, 16) and bytes(pub[0]) == bytes(16)
    assert [bytes(b) for b in pub[1:]] == [R.IV3 + (1 + i).to_bytes(4, "big") for i in range(n_blk + 1)]
    assert [bytes(b) for b in hashed] == R.hashed_blocks(aad, c)
    src, chunks = aes_var.gcm_tag_rows(R.IV3, aad, c, 16, 8)
    rows = R.tag_rows(aad, c, 16)
    assert list(src) == [len(r) for r in rows] and list(chunks) == [len(R.row_chunks(r)) for r in rows]
    if not aad_len and not data_len:  # m = 1, an all-zero length block: every row holds only its J0 bit
        assert hashed.shape == (1, 16) and not hashed.any() and not src.any() and set(chunks) == {1}


def test_counter_wraps_without_touching_the_iv():
    """The counter field is the low 32 bits: payload block 2^32 - 2 has counter 0 and the IV's last byte, 0xFF,
    stays.  A frame that long cannot be formatted in a test; the library forms be32(1 + i) in 32-bit arithmetic, and
    its blocks are compared here as far as a test can afford."""
    iv = bytes(11) + b"\xff"
    assert aes_var._gcm_counter_block(iv, 0xFFFFFFFD) == iv + b"\xff\xff\xff\xff"
    assert aes_var._gcm_counter_block(iv, 0xFFFFFFFE) == iv + bytes(4)
    assert aes_var._gcm_counter_block(iv, 0xFFFFFFFF) == iv + b"\x00\x00\x00\x01"
    pub, _ = aes_var.gcm_format(iv, b"", bytes(40), 16)
    assert [bytes(b) for b in pub[2:]] == [aes_var._gcm_counter_block(iv, i) for i in range(3)]
    assert bytes(pub[1]) == iv + b"\x00\x00\x00\x01"


def test_refusals():
    fmt = aes_var.gcm_format
    assert _code(lambda: fmt(bytes(16), b"", b"", 16)) == N.TAE_E_PARAM
    assert _code(lambda: fmt(bytes(8), b"", b"", 16)) == N.TAE_E_PARAM
    for t in (0, 3, 5, 7, 9, 11, 17):
        assert _code(lambda: fmt(R.IV3, b"", b"", t)) == N.TAE_E_PARAM
    for t in aes_var.GCM_TAG_LENGTHS:
        fmt(R.IV3, b"", b"", t)
    # m > n_powers, and a row beyond 64 chunks: 99 dense blocks are about 6400 sources a row
    assert _code(lambda: aes_var.gcm_tag_rows(R.IV3, bytes(16), bytes(16), 16, 2)) == N.TAE_E_PARAM
    aes_var.gcm_tag_rows(R.IV3, bytes(16), bytes(16), 16, 3)
    assert _code(lambda: aes_var.gcm_tag_rows(R.IV3, b"", bytes([0xA5]) * (99 * 16), 16, 128)) == N.TAE_E_NOISE
    src, chunks = aes_var.gcm_tag_rows(R.IV3, b"", bytes([0xA5]) * (40 * 16), 16, 64)
    assert max(chunks) <= 64 and max(chunks) == len(R.row_chunks(range(int(max(src)))))


def test_noise_schedule_check():
    for kb in aes_var.KEY_BITS:
        aes_var.gcm_noise_schedule_check(PID, kb, kb // 32 + 6, 5)
    aes_var.gcm_noise_schedule_check(PID, 128, 2, 16, aad_len=8, data_len=32)
    assert _code(lambda: aes_var.gcm_noise_schedule_check(PID, 128, 1, 4)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.gcm_noise_schedule_check(PID, 128, 11, 4)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.gcm_noise_schedule_check(PID, 128, 10, 0)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.gcm_noise_schedule_check(PID, 128, 10, 65)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.gcm_noise_schedule_check(PID, 160, 10, 4)) == N.TAE_E_PARAM
    assert _code(lambda: aes_var.gcm_noise_schedule_check(PID, 128, 10, 2)) == N.TAE_E_PARAM  # 8 + 17 bytes: m = 4
    assert _code(lambda: aes_var.gcm_noise_schedule_check(PID, 128, 10, 64, 0, 99 * 16)) == N.TAE_E_PARAM  # m = 100 > 64
    assert _code(lambda: aes_var.gcm_noise_schedule_check(tfhe_aes.PARAMS_WOPPBS_8BIT, 128, 10, 4)) == N.TAE_E_PARAM


def test_null_arguments():
    L = N.lib()
    key = np.zeros((44 * W, 4), dtype=np.uint64)
    out = np.zeros((128, 4), dtype=np.uint64)
    n = C.c_size_t(0)
    iv = np.zeros(12, dtype=np.uint8)
    assert L.tae_aesx_gcm_format(None, 12, None, 0, None, 0, 16, C.byref(n), C.byref(n), None, None) == N.TAE_E_ARG
    assert L.tae_aesx_gcm_format(_vp(iv), 12, None, 3, None, 0, 16, C.byref(n), C.byref(n), None, None) == N.TAE_E_ARG
    assert L.tae_aesx_ghash_key_raw(None, 128, None, 4, 10, _vp(out), N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_aesx_ghash_key_raw(None, 160, _vp(key), 4, 10, _vp(out), N.TAE_MEM_HOST) == N.TAE_E_PARAM
    arr, _keep, _ = aes_var._gcm_frames([(bytes(12), b"", bytes(16))], 16)
    assert L.tae_aesx_gcm_transcipher_raw(None, 128, _vp(key), None, 1, arr, 1, 16, 10, _vp(out), _vp(out),
                                          N.TAE_MEM_HOST) == N.TAE_E_ARG
    assert L.tae_stage_gf128_product(None, _vp(out), None, 1, _vp(out), N.TAE_MEM_HOST) == N.TAE_E_ARG


# ---- the noise table of DESIGN.md 5.14, from the byte-wise times_x alone ----------------------------------------
def test_design_table():
    sq = R.square_rows()
    assert max(len(r) for r in sq) == 5 and abs(sum(len(r) for r in sq) / 128 - 2.6) < 0.05
    chunks, chunk_t, reduce, per_t = R.product_plan()
    assert max(per_t) == 63 and sum(per_t) == 7168 and len(per_t) == 255
    assert len(chunks) == 1135 and max(len(c) for c in chunks) == 7 and 7 * 8 <= 64
    assert sorted(s for c in chunks for s in c) == list(range(7168))  # every partial bit once
    xp = [R.coefs(v) for v in R.x_pows()]
    assert max(sum(xp[t][r] for t in range(255)) for r in range(128)) == 8  # the reduction 255 -> 128
    assert max(len(r) for r in reduce) == 34 and max(len(r) for r in reduce) <= 64
    rnd = random.Random(11)
    weights = []
    for _ in range(4):
        x = bytes(rnd.randrange(256) for _ in range(16))
        weights += [len(r) for r in R.tag_rows(b"", x, 16)]  # one dense block and the sparse length block
    assert 51 - 3 <= min(weights) and max(weights) <= 72 + 3 + 9  # the issue's 51 .. 72 of 128, plus the length block
    # by bootstrap count: 8192 bit bootstraps and 1135 + 128 refreshes a product, against 1280 a block
    assert abs((8192 + 1135 + 128) / 1280 - 7.4) < 0.05
    assert R.power_schedule(5) == [([2], []), ([4], [3]), ([], [5])]


# ---- the host layer, compiled stand-alone -----------------------------------------------------------------------
@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")),
                         ids=("plain", "sanitized"))
def test_gcm_layer_native(tmp_path, flags):
    exe = str(tmp_path / "aes_gcm_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "aes_gcm_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_noise_levels_and_ids_native(tmp_path):
    exe = str(tmp_path / "aes_gcm_noise_test")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tfhe-aes-2_amd")], check=True)
    lib = os.path.join(ROOT, "tfhe-aes-2_amd", "tfhe_aes")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "aes_gcm_noise_test.cpp"),
                    os.path.join(lib, "libtfhe_aes_amd.so"), "-o", exe, "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
